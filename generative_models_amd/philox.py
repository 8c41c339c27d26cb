"""csrc/gm_philox.h read in numpy: the counter-based generator every device-drawn noise stream of the VAE family uses, for
the models' `*_reference` functions (what the tests compare the kernels with, bit for bit).

The layout.  Philox4x32-10 under key (seed mod 2^32, seed >> 32) at counter (e >> 2, step, row, tag) gives word e & 3 to
element e of row `row`: an element's word depends on (seed, step, row, tag, e) alone, never on the work mapping.  A word w
becomes a uniform in (0, 1) as (2 (w >> 9) + 1) 2^-24, and a group of four words two Box-Muller pairs (0, 1), (2, 3)."""
import numpy as np

_M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox4x32-10 over arrays: ctr [..., 4] and key [..., 2] (broadcast) of uint32 -> [..., 4] uint32."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) for i in range(4)]
    k0 = np.asarray(key[..., 0], dtype=np.uint64)
    k1 = np.asarray(key[..., 1], dtype=np.uint64)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & np.uint64(_M32), p1 & np.uint64(_M32),
             ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & np.uint64(_M32), p0 & np.uint64(_M32)]
        k0 = (k0 + np.uint64(0x9E3779B9)) & np.uint64(_M32)
        k1 = (k1 + np.uint64(0xBB67AE85)) & np.uint64(_M32)
    return np.stack(c, axis=-1).astype(np.uint32)


def words(n, width, seed, step, tag, row0=0):
    """The uint32 word of elements 0 .. width - 1 of rows row0 .. row0 + n - 1 at `step` under `tag`: [n, width]."""
    nq = (width + 3) // 4
    ctr = np.zeros((n, nq, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(nq, dtype=np.uint64)[None, :]
    ctr[..., 1] = np.uint64(int(step) & _M32)
    ctr[..., 2] = ((np.arange(n, dtype=np.uint64) + np.uint64(row0)) & np.uint64(_M32))[:, None]
    ctr[..., 3] = np.uint64(int(tag) & _M32)
    key = np.array([seed & _M32, (seed >> 32) & _M32], dtype=np.uint64)
    return philox4x32_10(ctr, key).reshape(n, 4 * nq)[:, :width]


def unit_uniforms(w):
    """ph_unit of every word: (2 (w >> 9) + 1) 2^-24 in (0, 1), float32 (exact: 24 significant bits)."""
    w = np.asarray(w).astype(np.uint64)
    return ((2 * (w >> np.uint64(9)) + 1).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def box_muller_normals(words):
    """The normal of every word ([n, 4k] uint32: pairs (0, 1), (2, 3) of each group of four), float64."""
    u = ((2.0 * (words >> np.uint32(9)).astype(np.float64) + 1.0) * 2.0 ** -24)
    w = u.reshape(u.shape[0], -1, 2)
    r = np.sqrt(-2.0 * np.log(w[..., 0]))
    phi = 2.0 * np.pi * w[..., 1]
    return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=-1).reshape(u.shape)


def normals(n, width, seed, step, tag, row0=0):
    """The normals of elements 0 .. width - 1 of rows row0 ..: [n, width] float64 (whole groups of four are drawn)."""
    return box_muller_normals(words(n, 4 * ((width + 3) // 4), seed, step, tag, row0))[:, :width]
