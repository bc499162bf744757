"""The scalar fp32 routines of k_mlp_tt's side work (gen_mlp_tt.py), transcribed from what hipcc emits for the same C++: one value
per lane, temporaries named by register number.  Each takes the emitter (tt_emit.Emitter) and VGPR numbers, and emits text only.
(div and sqrt have no caller while |d| and d / |d| come from k_ray_aux's per-ray table.)"""
import struct

from tt_regs import S_K, S_T0


def f32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def div(em, res, num, den, t):
    """res = num / den, correctly rounded (the sequence hipcc emits for -fhip-fp32-correctly-rounded-divide-sqrt); t: 5 temps"""
    a, r, b, q_, x = t[:5]
    e = em.e
    e("v_div_scale_f32 v%d, s[%d:%d], v%d, v%d, v%d" % (a, S_T0 + 0, S_T0 + 1, den, den, num))
    e("v_rcp_f32 v%d, v%d" % (r, a))
    e("v_div_scale_f32 v%d, vcc, v%d, v%d, v%d" % (b, num, den, num))
    e("v_fma_f32 v%d, -v%d, v%d, 1.0" % (x, a, r))
    e("v_fmac_f32 v%d, v%d, v%d" % (r, x, r))
    e("v_mul_f32 v%d, v%d, v%d" % (q_, b, r))
    e("v_fma_f32 v%d, -v%d, v%d, v%d" % (x, a, q_, b))
    e("v_fmac_f32 v%d, v%d, v%d" % (q_, x, r))
    e("v_fma_f32 v%d, -v%d, v%d, v%d" % (a, a, q_, b))
    e("v_div_fmas_f32 v%d, v%d, v%d, v%d" % (a, a, r, q_))
    e("v_div_fixup_f32 v%d, v%d, v%d, v%d" % (res, a, den, num))


def sqrt(em, res, x, t):
    """res = sqrtf(x), correctly rounded (hipcc's sequence); x is clobbered; t: 3 temps"""
    y, ym, tt = t[:3]
    e = em.e
    em.lit(S_K, 0x0f800000)
    e("v_mul_f32 v%d, 0x4f800000, v%d" % (tt, x))
    e("v_cmp_gt_f32 vcc, s%d, v%d" % (S_K, x))
    e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (x, x, tt))
    e("v_sqrt_f32 v%d, v%d" % (y, x))
    e("s_nop 0")
    e("v_add_u32 v%d, -1, v%d" % (ym, y))
    e("v_fma_f32 v%d, -v%d, v%d, v%d" % (tt, ym, y, x))
    e("v_cmp_ge_f32 s[%d:%d], 0, v%d" % (S_T0, S_T0 + 1, tt))
    e("v_cndmask_b32 v%d, v%d, v%d, s[%d:%d]" % (ym, y, ym, S_T0, S_T0 + 1))
    e("v_add_u32 v%d, 1, v%d" % (tt, y))
    e("v_fma_f32 v%d, -v%d, v%d, v%d" % (y, tt, y, x))
    e("v_cmp_lt_f32 s[%d:%d], 0, v%d" % (S_T0, S_T0 + 1, y))
    e("v_cndmask_b32 v%d, v%d, v%d, s[%d:%d]" % (ym, ym, tt, S_T0, S_T0 + 1))
    e("v_mul_f32 v%d, 0x37800000, v%d" % (tt, ym))
    e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (ym, ym, tt))
    e("v_mov_b32 v%d, 0x260" % tt)
    e("v_cmp_class_f32 vcc, v%d, v%d" % (x, tt))
    e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (res, ym, x))


def sincos(em, s_out, c_out, x, t):
    """sincos_cw (pnr_mlp.hip): s_out, c_out = sin, cos of v[x]; t: 6 temps"""
    kf, r, r2, a, b, ki = t[:6]
    e = em.e
    C = dict(twoopi=f32(0.636619772367581343), c1=f32(1.57079637050628662109375), c2=f32(-4.371139000186241e-08),
             s3=f32(-1.9515295891e-4), s2=f32(8.3321608736e-3), s1=f32(-1.6666654611e-1),
             c4=f32(2.443315711809948e-5), c3=f32(-1.388731625493765e-3), c2b=f32(4.166664568298827e-2))
    assert C["twoopi"] == 0x3f22f983 and C["c1"] == 0x3fc90fdb and C["c2"] == 0xb33bbd2e and C["s3"] == 0xb94ca1f9
    assert C["s2"] == 0x3c08839e and C["s1"] == 0xbe2aaaa3 and C["c4"] == 0x37ccf5ce and C["c3"] == 0xbab6061a and C["c2b"] == 0x3d2aaaa5
    e("v_mul_f32 v%d, 0x%x, v%d" % (kf, C["twoopi"], x))
    e("v_rndne_f32 v%d, v%d" % (kf, kf))
    e("v_mov_b32 v%d, v%d" % (r, x))
    e("v_fmac_f32 v%d, 0x%x, v%d" % (r, C["c1"] ^ 0x80000000, kf))              # r = fma(kf, -C1, x) = fma(-kf, C1, x)
    e("v_fmac_f32 v%d, 0x%x, v%d" % (r, C["c2"] ^ 0x80000000, kf))              # r = fma(-kf, C2, r)
    e("v_cvt_i32_f32 v%d, v%d" % (ki, kf))
    e("v_mul_f32 v%d, v%d, v%d" % (r2, r, r))
    # sine polynomial
    e("v_mov_b32 v%d, 0x%x" % (a, C["s2"]))
    e("v_fmac_f32 v%d, 0x%x, v%d" % (a, C["s3"], r2))                           # sp = fma(r2, s3, s2)
    e("v_fmaak_f32 v%d, v%d, v%d, 0x%x" % (a, r2, a, C["s1"]))                  # sp = fma(r2, sp, s1)
    e("v_mul_f32 v%d, v%d, v%d" % (b, r, r2))                                   # r * r2
    e("v_fma_f32 v%d, v%d, v%d, v%d" % (a, b, a, r))                            # sn = fma(r * r2, sp, r)
    # cosine polynomial
    e("v_mov_b32 v%d, 0x%x" % (b, C["c3"]))
    e("v_fmac_f32 v%d, 0x%x, v%d" % (b, C["c4"], r2))                           # cp = fma(r2, c4, c3)
    e("v_fmaak_f32 v%d, v%d, v%d, 0x%x" % (b, r2, b, C["c2b"]))                 # cp = fma(r2, cp, c2)
    e("v_fma_f32 v%d, v%d, v%d, -0.5" % (b, r2, b))                             # cp = fma(r2, cp, -0.5)
    e("v_fma_f32 v%d, v%d, v%d, 1.0" % (b, r2, b))                              # cs = fma(r2, cp, 1)
    # quadrant
    e("v_and_b32 v%d, 1, v%d" % (r, ki))
    e("v_cmp_eq_u32 vcc, 0, v%d" % r)
    e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (r2, b, a))                          # so = (k & 1) ? cs : sn
    e("v_cndmask_b32 v%d, v%d, v%d, vcc" % (kf, a, b))                          # co = (k & 1) ? sn : cs
    e("v_and_b32 v%d, 2, v%d" % (a, ki))
    e("v_lshlrev_b32 v%d, 30, v%d" % (a, a))
    e("v_xor_b32 v%d, v%d, v%d" % (s_out, r2, a))                               # s = so ^ ((k & 2) << 30)
    e("v_add_u32 v%d, 1, v%d" % (a, ki))
    e("v_and_b32 v%d, 2, v%d" % (a, a))
    e("v_lshlrev_b32 v%d, 30, v%d" % (a, a))
    e("v_xor_b32 v%d, v%d, v%d" % (c_out, kf, a))                               # c = co ^ (((k + 1) & 2) << 30)


def band_pack(em, dst3, s, c):
    """three packed registers of one band: (s_x s_y) (s_z c_x) (c_y c_z)"""
    e = em.e
    e("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (dst3, s[0], s[1]))
    e("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (dst3 + 1, s[2], c[0]))
    e("v_cvt_pk_bf16_f32 v%d, v%d, v%d" % (dst3 + 2, c[1], c[2]))


def band_next(em, s, c, t):
    """double-angle step, in place: s2 = (2 s) c, c2 = fma(-2 s, s, 1)"""
    e = em.e
    for a in range(3):
        e("v_add_f32 v%d, v%d, v%d" % (t, s[a], s[a]))                          # 2 s (exact)
        e("v_mul_f32 v%d, v%d, v%d" % (t, t, c[a]))                             # s2 = (2 s) * c
        e("v_mul_f32 v%d, -2.0, v%d" % (c[a], s[a]))                            # -2 s
        e("v_fma_f32 v%d, v%d, v%d, 1.0" % (c[a], c[a], s[a]))                  # c2 = fma(-2 s, s, 1)
        e("v_mov_b32 v%d, v%d" % (s[a], t))
