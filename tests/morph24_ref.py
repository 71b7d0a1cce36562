"""The 24-bit dense morph storage format in numpy (include/reze_deform.h: rz_upload_morphs_dense; DESIGN.md "Dense morph storage") — the
model the encoder (upload.cpp) and the device decode (kernels/common.hip.h) are held to, value for value.

Per morph: E = the binary exponent of the largest finite |delta| over its three planes, s = 2^(E - 22), q = rint(d / s) (ties to even);
if that takes the maximum to 2^23, E + 1. An all-zero morph: s = 1. Four consecutive values take three dwords — d0 = q0 | q1[7:0] << 24,
d1 = q1[23:8] | q2[15:0] << 16, d2 = q2[23:16] | q3 << 8 — which is each value's three bytes, low byte first, back to back. The whole set stays
fp32 when a delta is not finite or an exponent leaves [-64, 64]."""
import numpy as np


def exponents(deltas):
    """E_m per morph of deltas [M, V, 3], or None where the set stays fp32. An all-zero morph reports E = 22 (s = 1)."""
    d = np.asarray(deltas, dtype=np.float32)
    if not np.isfinite(d).all():
        return None
    out = []
    for m in range(d.shape[0]):
        mx = float(np.abs(d[m]).max()) if d[m].size else 0.0
        if mx == 0.0:
            out.append(22)
            continue
        E = int(np.frexp(mx)[1]) - 1                      # mx = f * 2^E, 1 <= f < 2 (a denormal's E is below -126: out of range below)
        if np.rint(np.ldexp(mx, 22 - E)) >= 2.0 ** 23:
            E += 1
        if E < -64 or E > 64:
            return None
        out.append(E)
    return np.array(out, dtype=np.int64)


def encode(deltas):
    """(storage, scales [M] float32, packed [M, 3, ceil(V / 4) * 12] uint8, decoded [M, 3, V] float32); storage 32: the rest is None."""
    d = np.asarray(deltas, dtype=np.float32)
    E = exponents(d)
    if E is None:
        return 32, None, None, None
    M, V = d.shape[0], d.shape[1]
    s = np.ldexp(1.0, E - 22)                             # float64, exact
    q = np.rint(d.astype(np.float64) / s[:, None, None]).astype(np.int64)       # [M, V, 3]
    assert np.abs(q).max(initial=0) < 2 ** 23
    planes = np.transpose(q, (0, 2, 1))                   # [M, 3, V]
    u = (planes & 0xffffff).astype(np.uint32)
    Vq = (V + 3) // 4 * 4
    by = np.zeros((M, 3, Vq, 3), dtype=np.uint8)
    by[:, :, :V, 0] = u & 0xff
    by[:, :, :V, 1] = (u >> 8) & 0xff
    by[:, :, :V, 2] = (u >> 16) & 0xff
    decoded = (planes.astype(np.float64) * s[:, None, None]).astype(np.float32)      # exact: 24 bits times a power of two
    return 24, s.astype(np.float32), by.reshape(M, 3, Vq * 3), decoded


def dwords_of_quad(q4):
    """The three dwords of four signed 24-bit values, written out as the header states them (a check of `encode`'s byte layout)."""
    q = [int(x) & 0xffffff for x in q4]
    return [q[0] | (q[1] & 0xff) << 24, q[1] >> 8 | (q[2] & 0xffff) << 16, q[2] >> 16 | q[3] << 8]
