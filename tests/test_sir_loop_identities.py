"""The arithmetic identities behind the one-lane SIR event loop (fast_propagate_sir, csrc/epipf_device.hpp;
DESIGN.md §4.2), checked in numpy float32 on random and edge inputs.  The loop carries D = 2S instead of S and takes
the channel from the sign bit of t = c0 * rcp(total) - uc; every lane must still take the decisions of the S-form
(FastSsa<kSIR, 1>::cum / apply), which the lane-group pass and the replay keep using."""
import numpy as np

f32 = np.float32
K_BAND = f32(2.0 ** -19)                                  # FastSsa<kSIR, 1>::kBand
ULP = f32(2.0 ** -24)


def fma32(a, b, c):
    """fl32(a * b + c) for float32 arrays: the product of two f32 is exact in f64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def rate_grid(rs, n):
    """Rates over rate_ok's range [2^-60, 2^40]: its ends, powers of two, random mantissas; and zero."""
    e = rs.randint(-60, 40, n)
    v = np.ldexp(rs.uniform(1.0, 2.0, n), e).astype(f32)
    v[:6] = [2.0 ** -60, 2.0 ** 40, 0.0, 1.0, np.nextafter(f32(2.0 ** -60), f32(1)), np.nextafter(f32(2.0 ** 40), f32(0))]
    return np.clip(v, 0, f32(2.0 ** 40))


def counts(rs, n):
    """(S, I) with S + I <= 2^24 - 1: random over every magnitude, and the edges."""
    top = 2 ** 24 - 1
    S = np.floor(np.exp2(rs.uniform(0, 24, n))).astype(np.int64)
    I = np.floor(np.exp2(rs.uniform(0, 24, n))).astype(np.int64)
    S[:8] = [0, 0, 1, top - 1, top, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1]
    I[:8] = [1, top, 1, 1, 0, 2 ** 23, 2 ** 23 - 1, 1]
    S = np.minimum(S, top)
    I = np.minimum(I, top - S)
    return S, I


def test_d_form_rate_and_total_equal_the_s_form_bit_for_bit():
    rs = np.random.RandomState(7)
    n = 400000
    S, I = counts(rs, n)
    bN, g = rate_grid(rs, n), rate_grid(rs, n)[::-1].copy()
    Sf, If, Df = S.astype(f32), I.astype(f32), (2 * S).astype(f32)
    assert np.array_equal(Df.astype(np.int64), 2 * S)                  # D is exact: an even integer below 2^25
    bNh = bN * f32(0.5)
    assert np.array_equal(bNh.astype(np.float64) * 2.0, bN.astype(np.float64))   # the halved rate is exact (normal)
    c_s = bN * (Sf * If)
    c_d = bNh * (Df * If)
    assert np.array_equal(bits(c_s), bits(c_d))
    assert np.array_equal(bits(fma32(g, If, c_s)), bits(fma32(g, If, c_d)))
    # the scaled rate as well: the smallest nonzero product stays normal (S I >= 1, bN >= 2^-60)
    nz = (c_s != 0)
    assert np.all(np.abs(c_s[nz]) >= f32(2.0 ** -60))


def test_event_updates_stay_exact_integers():
    rs = np.random.RandomState(8)
    n = 400000
    S, I = counts(rs, n)
    Df, If = (2 * S).astype(f32), I.astype(f32)
    for s in (f32(1.0), f32(-1.0)):                                    # +1 infection, -1 recovery
        ok = (S >= 1) if s > 0 else (I >= 1)
        step = f32(1.0) + s                                            # 0 or 2
        D1, I1 = Df - step, If + s
        assert np.array_equal(D1[ok].astype(np.int64), (2 * S - int(step))[ok])
        assert np.array_equal(I1[ok].astype(np.int64), (I + int(s))[ok])
        # the undo restores the state, and S = D / 2 is the S-form's count
        assert np.array_equal(bits(D1 + step), bits(Df))
        assert np.array_equal(bits(I1 - s), bits(If))
        assert np.array_equal((D1 * f32(0.5))[ok].astype(np.int64), (S - int(step) // 2)[ok])


def test_sign_bit_channel_equals_the_compare_outside_the_band():
    rs = np.random.RandomState(9)
    n = 1000000
    S, I = counts(rs, n)
    bN, g = rate_grid(rs, n), rate_grid(rs, n)[::-1].copy()
    Sf, If = S.astype(f32), I.astype(f32)
    c0 = bN * (Sf * If)
    total = fma32(g, If, c0)
    keep = (total > 0) & np.isfinite(total)
    c0, total = c0[keep], total[keep]
    m = c0.size
    with np.errstate(over="ignore"):
        ri = (f32(1.0) / total)
        # arbitrary reciprocals around the hardware's (v_rcp_f32 is within 1.53 ulp): a few ulp either way, and exact
        ri = (ri.view(np.int32) + rs.randint(-3, 4, m).astype(np.int32)).view(f32)
    ri = np.where(np.isfinite(ri) & (ri > 0), ri, f32(1.0) / total)
    w = rs.randint(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32)   # the Philox word r.w
    w[:4] = [0, 0xFFFFFFFF, 0x1FF, 0x200]
    # half the words next to the lane's own ratio, so that the band and its edges are exercised
    q0 = np.clip(c0 * ri, 0, 1 - 2.0 ** -24)
    near = (np.floor(q0.astype(np.float64) * 2 ** 23).astype(np.int64) + rs.randint(-40, 41, m)).clip(0, 2 ** 23 - 1)
    w = np.where(rs.rand(m) < 0.5, (near.astype(np.uint64) << np.uint64(9)).astype(np.uint32), w)
    a = ((w >> np.uint32(9)) | np.uint32(0x3F800000)).view(f32)
    b = f32(1.0) - ULP
    uc, nuc = a - b, b - a
    assert np.array_equal(bits(nuc), bits(-uc))                        # -uc from the same three operations, exact
    assert np.array_equal(uc.astype(np.float64), a.astype(np.float64) - (1.0 - 2.0 ** -24))
    q = c0 * ri
    old = q < uc                                                       # today's decision: True = recovery
    t2 = q - uc                                                        # two roundings
    tf = fma32(c0, ri, nuc)                                            # one rounding
    for t in (t2, tf):
        sure = np.abs(t) > K_BAND
        assert sure.sum() > m // 4 and (~sure).sum() > 1000
        s = np.copysign(f32(1.0), t)
        assert np.array_equal((s < 0)[sure], old[sure])
    # t = +0 (q == uc) reads as infection, as q < uc does
    z = np.copysign(f32(1.0), f32(0.5) - f32(0.5))
    assert z == 1.0
    # the two forms differ by at most an ulp of q: inside the e_q bound of the band
    assert np.all(np.abs(t2.astype(np.float64) - tf.astype(np.float64)) <= np.spacing(np.maximum(q, uc)).astype(np.float64))
