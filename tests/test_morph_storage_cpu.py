"""The 24-bit dense morph encoder (upload.cpp, through rz_morph_encode24: host only, no device) against the numpy model of the format
(tests/morph24_ref.py): packed bytes value for value, scales, the fp32 fallback, and the error bound 2^(E - 23) of every stored value."""
import numpy as np
import pytest

import morph24_ref as ref


def both(rz, deltas):
    d = np.ascontiguousarray(deltas, dtype=np.float32)
    st, sc, pk = rz.capi.morph_encode24(d)
    rst, rsc, rpk, dec = ref.encode(d)
    assert st == rst
    if st == 24:
        assert np.array_equal(sc, rsc), (sc, rsc)
        assert np.array_equal(pk, rpk)
    return st, sc, pk, dec


def assert_bound(deltas, dec):
    d = np.asarray(deltas, dtype=np.float32)
    E = ref.exponents(d)
    err = np.abs(np.transpose(dec, (0, 2, 1)).astype(np.float64) - d.astype(np.float64))
    bound = np.ldexp(1.0, E - 23)[:, None, None]
    assert (err <= bound).all(), float((err / bound).max())


def test_model_byte_layout_is_the_dword_layout_of_the_header():
    rng = np.random.default_rng(5)
    q = rng.integers(-2 ** 23 + 1, 2 ** 23, size=(50, 4))
    for row in q:
        d = (row.astype(np.float64) * 2.0 ** -22).astype(np.float32)[None, :, None].repeat(3, axis=2)      # one morph, V = 4
        d[0, 0, :] = np.float32((2 ** 23 - 1) * 2.0 ** -22)          # pins E = 0, s = 2^-22
        st, s, by, _ = ref.encode(d)
        assert st == 24 and s[0] == np.float32(2.0 ** -22)
        qq = np.rint(d[0, :, 0].astype(np.float64) * 2.0 ** 22).astype(np.int64)
        assert by[0, 0].view("<u4").tolist() == ref.dwords_of_quad(qq)


@pytest.mark.parametrize("V", [1, 3, 4, 5, 31, 33, 127, 129, 1021])
def test_encoder_matches_the_model_on_ragged_sizes(rz, V):
    rng = np.random.default_rng(100 + V)
    d = ((rng.random((5, V, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1)).astype(np.float32)
    st, _sc, pk, dec = both(rz, d)
    assert st == 24 and pk.shape == (5, 3, (V + 3) // 4 * 12)
    assert_bound(d, dec)


def test_edge_inputs_range_and_scale(rz):
    rng = np.random.default_rng(7)
    V = 37
    base = ((rng.random((V, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1)).astype(np.float32)
    zero = np.zeros((V, 3), dtype=np.float32)
    pow_pos = base.copy(); pow_pos[3, 1] = np.float32(0.25)             # max exactly +2^k
    pow_neg = base.copy(); pow_neg[9, 2] = np.float32(-0.5)             # max exactly -2^k
    bump = base.copy(); bump[5, 0] = np.nextafter(np.float32(0.125), np.float32(0))      # mantissa all ones: rounds to 2^23, so E + 1
    bump_neg = base.copy(); bump_neg[6, 2] = -np.nextafter(np.float32(0.25), np.float32(0))
    outlier = (base * np.float32(0.02)).astype(np.float32); outlier[11, 1] = np.float32(1e3)    # one 1e3 among ~1e-3 values
    d = np.stack([zero, pow_pos, pow_neg, bump, bump_neg, outlier])
    st, sc, pk, dec = both(rz, d)
    assert st == 24
    E = ref.exponents(d)
    assert E.tolist() == [22, -2, -1, -3, -2, 9]
    assert sc.tolist() == [1.0, 2.0 ** -24, 2.0 ** -23, 2.0 ** -25, 2.0 ** -24, 2.0 ** -13]
    assert not pk[0].any() and not dec[0].any()
    assert dec[1][1, 3] == np.float32(0.25) and dec[2][2, 9] == np.float32(-0.5)
    assert dec[3][0, 5] == np.float32(0.125) and dec[4][2, 6] == np.float32(-0.25)      # the bumped maxima land on the power of two
    assert dec[5][1, 11] == np.float32(1e3)
    assert_bound(d, dec)
    # every stored integer is inside the signed 24-bit range
    q = np.rint(np.transpose(dec, (0, 2, 1)).astype(np.float64) / sc.astype(np.float64)[:, None, None])
    assert np.abs(q).max() <= 2 ** 23 - 1


def test_fallback_to_fp32(rz):
    rng = np.random.default_rng(9)
    good = ((rng.random((3, 21, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(0.1)).astype(np.float32)
    assert both(rz, good)[0] == 24
    for bad in (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)):
        d = good.copy(); d[1, 4, 2] = bad
        assert both(rz, d)[0] == 32
    den = np.zeros((2, 21, 3), dtype=np.float32); den[0] = good[0]; den[1, 2, 0] = np.float32(1e-40)      # a denormal maximum
    assert both(rz, den)[0] == 32
    tiny = good.copy(); tiny[2] = np.float32(2.0 ** -70) * np.sign(good[2])                               # exponent below -64
    assert both(rz, tiny)[0] == 32
    huge = good.copy(); huge[0, 0, 0] = np.float32(2.0 ** 66)
    assert both(rz, huge)[0] == 32
    edge_lo = good.copy(); edge_lo[2] = np.float32(2.0 ** -64) * np.sign(good[2]); edge_lo[2, 0, 0] = np.float32(2.0 ** -64)
    edge_hi = good.copy(); edge_hi[0, 0, 0] = np.float32(2.0 ** 64)
    assert both(rz, edge_lo)[0] == 24 and both(rz, edge_hi)[0] == 24      # [-64, 64] itself is inside


def test_entry_points_are_declared(rz):
    L = rz.capi.load()
    for name in ("rz_upload_morphs_dense_ex", "rz_read_morph_dense", "rz_morph_encode24"):
        assert hasattr(L, name) and name in rz.capi.SYMBOLS and name in rz.capi.OPTIONAL_SYMBOLS
    assert rz.capi.MORPH_F32 == 1
