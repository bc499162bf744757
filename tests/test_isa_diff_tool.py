"""tools/isa_diff.py on two tiny synthetic builds (no GPU, no hipcc): a kernel whose template parameter list lost a parameter
is "missing" by name, matches under --rename, and a changed body is still reported DIFFERENT under the new name."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "isa_diff.py")

OLD_NAME = "_Z11k_mlp_fusedILi1ELi256ELi1ELi8ELi2ELb1EEvPf"      # k_mlp_fused<1, 256, 1, 8, 2, true>(float*)
NEW_NAME = "_Z11k_mlp_fusedILi1ELi256ELi8ELi2ELb1EEvPf"          # k_mlp_fused<1, 256, 8, 2, true>(float*)
OTHER = "_Z9k_ray_auxPKflPj"                                       # k_ray_aux(float const*, long, unsigned int*): same name in both
RENAME = r"k_mlp_fused<(\d+), (\d+), 1, =k_mlp_fused<\1, \2, "
BODY = ["s_load_dwordx2 s[0:1], s[4:5], 0x0", "s_waitcnt lgkmcnt(0)", "v_mov_b32_e32 v1, 0", "global_store_dword v1, v0, s[0:1]", "s_endpgm"]


def write_build(path, kernels):
    os.makedirs(path)
    text = ["\t.text"]
    for i, (name, body) in enumerate(kernels):
        text += ["\t.globl\t%s" % name, "%s:                      ; @%s" % (name, name), "; %%bb.0:"]
        text += ["\t" + line for line in body] + [".Lfunc_end%d:" % i, "\t.size\t%s, .Lfunc_end%d-%s" % (name, i, name)]
    with open(os.path.join(path, "x-hip-amdgcn-amd-amdhsa-gfx950.s"), "w") as f:
        f.write("\n".join(text) + "\n")


def run(*args):
    p = subprocess.run([sys.executable, TOOL, *args], capture_output=True, text=True)
    return p.returncode, p.stdout


def test_rename_matches_a_kernel_whose_template_parameters_changed(tmp_path):
    old, new, changed = str(tmp_path / "old"), str(tmp_path / "new"), str(tmp_path / "changed")
    write_build(old, [(OLD_NAME, BODY), (OTHER, BODY)])
    write_build(new, [(NEW_NAME, BODY), (OTHER, BODY)])
    write_build(changed, [(NEW_NAME, BODY[:2] + ["v_mov_b32_e32 v1, 1"] + BODY[3:]), (OTHER, BODY)])

    rc, out = run(old, new)                                         # by name alone: the old kernel is gone, a new one appeared
    assert rc == 1, out
    assert "missing   k_mlp_fused<1, 256, 1, 8, 2, true>(float*)" in out
    assert "new       k_mlp_fused<1, 256, 8, 2, true>(float*)" in out
    assert "same      k_ray_aux(" in out

    rc, out = run("--rename", RENAME, old, new)                     # with the option: the same kernel, the same code
    assert rc == 0, out
    assert "same      k_mlp_fused<1, 256, 8, 2, true>(float*) (5 lines)" in out
    assert "missing  " not in out and "new  " not in out and "DIFFERENT" not in out
    assert "2 kernel(s) of the old build: 2 identical, 0 different or missing" in out

    rc, out = run("--rename", RENAME, old, changed)                 # ... and a changed body is still found under the new name
    assert rc == 1, out
    assert "DIFFERENT k_mlp_fused<1, 256, 8, 2, true>(float*) (5 -> 5 lines)" in out
    assert "same      k_ray_aux(" in out
