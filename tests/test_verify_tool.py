"""tools/verify_against_reference.py must keep working until the real `panopticnerf` branch can be mounted (SURVEY.md 9;
VERDICT r1 item 8): run it against (a) a stub checkout that holds only a README (what the mounted reference is today) and
(b) a MOCK checkout laid out like the reference (lib/networks/renderer/..., lib/networks/<net>/network.py) whose helpers
wrap this repo's own oracle under the canonical nerf-pytorch signatures -- first unchanged (every check must agree), then
with one parity-critical constant altered (the tool must say which function differs)."""
import os
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import verify_against_reference as vt  # noqa: E402

MOCK_UTILS = '''
import sys, torch
sys.path.insert(0, %r)
from lib.config import cfg                      # the reference's modules read its global config
from oracle import torch_oracle as _to

def sample_pdf(bins, weights, N_samples, det=False):
    zs, _ = _to.sample_pdf(bins, weights, N_samples, det=True)
    return zs

def raw2outputs(raw, z_vals, rays_d, raw_noise_std=0, white_bkgd=False):
    o = _to.raw2outputs(raw, z_vals, rays_d)
    dists = z_vals[..., 1:] - z_vals[..., :-1]
    dists = torch.cat([dists, torch.full_like(dists[..., :1], %s)], -1)
    return o["rgb"] * (1.0 if %s == 1e10 else 1.001), o["depth"], o["acc"], o["weights"], o["depth"]
'''
MOCK_NET = '''
import torch
from oracle import torch_oracle as _to

def get_embedder(multires, input_dims=3):
    return (lambda x: _to.embed(x, multires)), 3 + 6 * multires

class Network(torch.nn.Module):
    pass
'''


def _mock(tmp_path, last_dist):
    r = tmp_path / "ref"
    (r / "lib" / "networks" / "renderer").mkdir(parents=True)
    (r / "lib" / "networks" / "nerf").mkdir(parents=True)
    (r / "lib" / "networks" / "renderer" / "nerf_net_utils.py").write_text(textwrap.dedent(MOCK_UTILS % (ROOT, last_dist, last_dist)))
    (r / "lib" / "networks" / "nerf" / "network.py").write_text(textwrap.dedent(MOCK_NET))
    (r / "lib" / "networks" / "renderer" / "make_renderer.py").write_text("import imp\ndef make_renderer(cfg, network):\n    return imp.load_source(cfg.renderer_module, cfg.renderer_path).Renderer(network)\n")
    return str(r)


def test_stub_reference_is_reported_not_crashed(tmp_path, capsys):
    stub = tmp_path / "stub"
    stub.mkdir()
    (stub / "README.md").write_text("# PanopticNeRF\n\nThe code lives on the `panopticnerf` and `panopticnerf360` branches.\n")
    assert vt.main([str(stub)]) == 2
    assert "nothing to verify" in capsys.readouterr().out


def test_mock_checkout_agrees_and_a_changed_constant_is_caught(tmp_path, capsys):
    for k in [m for m in sys.modules if m == "lib" or m.startswith("lib.") or m.startswith("_ref_")]:
        del sys.modules[k]
    rc = vt.main([_mock(tmp_path / "a", "1e10")])
    out = capsys.readouterr().out
    assert rc == 0, out
    assert "def sample_pdf" in out and "nerf_net_utils.py:" in out and "class Network" in out and "const 1e10" in out
    assert "z_samples (det)" in out and "gamma(x), L=10" in out and "0 differ" in out
    for k in [m for m in sys.modules if m == "lib" or m.startswith("lib.") or m.startswith("_ref_")]:
        del sys.modules[k]
    rc = vt.main([_mock(tmp_path / "b", "1e9")])          # a reference whose rgb differs: must be reported
    out = capsys.readouterr().out
    assert rc == 1 and "raw2outputs.rgb" in out
