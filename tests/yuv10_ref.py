"""The 10-bit 4:2:0 conversion contract of include/vtx_yuv10.h, restated in NumPy from the header's text alone (no kernel code
was read for it): planes of 16-bit words with byte pitches, a sample shift and a mask -> uint8 RGB.  tests/test_yuv10_host.py
holds its premises -- float64 matrices over the sample set S, the x4 identity with tests/yuv_ref.py over all 2^24 8-bit
triples --; tests/test_gpu_yuv10.py holds the kernels against it."""
import functools

import numpy as np

#: the header's table: (matrix, full_range) -> y_off, c_y, c_rv, c_gu, c_gv, c_bu, 12 fractional bits
PRESETS = {('bt601', False): (64, 1192, 1634, 401, 832, 2066), ('bt709', False): (64, 1192, 1836, 218, 546, 2163),
           ('bt601', True): (0, 1021, 1431, 351, 729, 1809), ('bt709', True): (0, 1021, 1608, 191, 478, 1895)}
#: luma weights (Kr, Kb) of the two standards, for the float64 form
LUMA = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}


def convert(Y, U, V, matrix):
    """Integer arrays of one shape, values 0 .. 1023 -> uint8 [..., 3]: the three formulas of the header in int32; ``>> 12`` on a
    NumPy int32 is the arithmetic shift (floor, also for negative sums)."""
    y_off, c_y, c_rv, c_gu, c_gv, c_bu = (np.int32(c) for c in matrix)
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    C, D, E = (Y - y_off) * c_y + np.int32(2048), U - np.int32(512), V - np.int32(512)
    R = (C + c_rv * E) >> 12
    G = (C - c_gu * D - c_gv * E) >> 12
    B = (C + c_bu * D) >> 12
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8)


def convert_f64(Y, U, V, matrix, full_range):
    """The standard's float64 matrix on 10-bit samples, rounded once (half up) and clamped -> uint8 [..., 3].  Limited range:
    luma 64 .. 940 scaled by 255 / 876, chroma by 255 / 896; full range: 255 / 1023 for both."""
    kr, kb = LUMA[matrix] if isinstance(matrix, str) else matrix
    kg = 1.0 - kr - kb
    Y, U, V = (np.asarray(a).astype(np.float64) for a in (Y, U, V))
    if full_range:
        y, cb, cr = Y * (255.0 / 1023.0), (U - 512.0) * (255.0 / 1023.0), (V - 512.0) * (255.0 / 1023.0)
    else:
        y, cb, cr = (Y - 64.0) * (255.0 / 876.0), (U - 512.0) * (255.0 / 896.0), (V - 512.0) * (255.0 / 896.0)
    R = y + 2.0 * (1.0 - kr) * cr
    B = y + 2.0 * (1.0 - kb) * cb
    G = y - (2.0 * kb * (1.0 - kb) / kg) * cb - (2.0 * kr * (1.0 - kr) / kg) * cr
    return np.clip(np.floor(np.stack([R, G, B], axis=-1) + 0.5), 0, 255).astype(np.uint8)


def planes_to_rgb(ybuf, ubuf, vbuf, shape, y_pitch, y_frame, c_pitch, c_frame, c_step, shift, matrix, y0=0, u0=0, v0=0):
    """Flat uint16 buffers addressed as the header says -> uint8 [Ts,Hs,Ws,3].  Pitches, frame strides and the three base offsets
    are BYTES (all even), c_step is SAMPLES: the luma word of pixel (t, s, x) lies at byte y0 + t * y_frame + s * y_pitch + 2 * x
    of ybuf, its chroma words at byte u0 / v0 + t * c_frame + (s >> 1) * c_pitch + 2 * (x >> 1) * c_step of ubuf / vbuf; a sample
    is (word >> shift) & 1023."""
    Ts, Hs, Ws = shape
    assert not (y_pitch | y_frame | c_pitch | c_frame | y0 | u0 | v0) & 1
    t, s, x = np.meshgrid(np.arange(Ts), np.arange(Hs), np.arange(Ws), indexing='ij')
    yi = (y0 + t * y_frame + s * y_pitch + 2 * x) >> 1
    ci = t * c_frame + (s >> 1) * c_pitch + 2 * (x >> 1) * c_step
    word = lambda buf, i: (np.asarray(buf).reshape(-1).view(np.uint16)[i].astype(np.int32) >> shift) & 1023
    return convert(word(ybuf, yi), word(ubuf, (u0 + ci) >> 1), word(vbuf, (v0 + ci) >> 1), matrix)


def clip_to_rgb(y, u, v=None, matrix=PRESETS[('bt601', False)], shift=None):
    """Contiguous 16-bit arrays: y [Ts,Hs,Ws]; yuv420p10le: u, v [Ts,Hc,Wc]; P010 (v None): u [Ts,Hc,Wc,2] -> uint8 [Ts,Hs,Ws,3].
    ``shift`` None: 6 for P010 (the sample in the upper 10 bits), 0 for the planar layout."""
    y, u = np.ascontiguousarray(y), np.ascontiguousarray(u)
    Ts, Hs, Ws = y.shape
    Hc, Wc = (Hs + 1) // 2, (Ws + 1) // 2
    if v is None:
        assert u.shape == (Ts, Hc, Wc, 2)
        return planes_to_rgb(y, u, u, (Ts, Hs, Ws), 2 * Ws, 2 * Hs * Ws, 4 * Wc, 4 * Hc * Wc, 2, 6 if shift is None else shift, matrix, v0=2)
    v = np.ascontiguousarray(v)
    assert u.shape == v.shape == (Ts, Hc, Wc)
    return planes_to_rgb(y, u, v, (Ts, Hs, Ws), 2 * Ws, 2 * Hs * Ws, 2 * Wc, 2 * Hc * Wc, 1, 0 if shift is None else shift, matrix)


GRID = np.unique(np.r_[np.arange(0, 1024, 5), 1023, 511:514, 63:66, 939:942, 959:962])


@functools.lru_cache(maxsize=None)
def sample_set():
    """The set S the presets are held against -> three int32 arrays (Y, U, V): 2^24 triples drawn from
    np.random.RandomState(0).randint(0, 1024, n) as Y, then U, then V, followed by the full grid GRID^3, which holds both range
    ends, the chroma centre and the limited-range bounds (64, 940 luma; 960 chroma) with their neighbours."""
    rs, n = np.random.RandomState(0), 1 << 24
    ry, ru, rv = (rs.randint(0, 1024, n).astype(np.int32) for _ in range(3))
    gy, gu, gv = (a.reshape(-1).astype(np.int32) for a in np.meshgrid(GRID, GRID, GRID, indexing='ij'))
    return np.concatenate([ry, gy]), np.concatenate([ru, gu]), np.concatenate([rv, gv])
