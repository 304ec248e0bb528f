"""The 4:2:0 conversion contract of include/vtx_yuv.h, restated in NumPy from the header's text alone (no kernel code was
read for it): planes with pitches -> uint8 RGB.  tests/test_yuv_host.py holds its premises -- grey axis, float64 matrices,
Pillow -- over all 2^24 triples; tests/test_gpu_yuv.py holds the kernels against it."""
import numpy as np

#: the header's table: (matrix, full_range) -> y_off, c_y, c_rv, c_gu, c_gv, c_bu
PRESETS = {('bt601', False): (16, 298, 409, 100, 208, 516), ('bt709', False): (16, 298, 459, 55, 136, 541),
           ('bt601', True): (0, 256, 359, 88, 183, 454), ('bt709', True): (0, 256, 403, 48, 120, 475)}
#: luma weights (Kr, Kb) of the two standards, for the float64 form
LUMA = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722)}


def convert(Y, U, V, matrix):
    """Integer arrays of one shape -> uint8 [..., 3]: the three formulas of the header in int32; ``>> 8`` on a NumPy int32 is
    the arithmetic shift (floor, also for negative sums)."""
    y_off, c_y, c_rv, c_gu, c_gv, c_bu = (np.int32(c) for c in matrix)
    Y, U, V = (np.asarray(a).astype(np.int32) for a in (Y, U, V))
    C, D, E = (Y - y_off) * c_y, U - np.int32(128), V - np.int32(128)
    R = (C + c_rv * E + np.int32(128)) >> 8
    G = (C - c_gu * D - c_gv * E + np.int32(128)) >> 8
    B = (C + c_bu * D + np.int32(128)) >> 8
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8)


def convert_f64(Y, U, V, matrix, full_range):
    """The standard's float64 matrix, rounded once (half up) and clamped -> uint8 [..., 3]."""
    kr, kb = LUMA[matrix]
    kg = 1.0 - kr - kb
    Y, U, V = (np.asarray(a).astype(np.float64) for a in (Y, U, V))
    if full_range:
        y, cb, cr = Y, U - 128.0, V - 128.0
    else:
        y, cb, cr = (Y - 16.0) * (255.0 / 219.0), (U - 128.0) * (255.0 / 224.0), (V - 128.0) * (255.0 / 224.0)
    R = y + 2.0 * (1.0 - kr) * cr
    B = y + 2.0 * (1.0 - kb) * cb
    G = y - (2.0 * kb * (1.0 - kb) / kg) * cb - (2.0 * kr * (1.0 - kr) / kg) * cr
    return np.clip(np.floor(np.stack([R, G, B], axis=-1) + 0.5), 0, 255).astype(np.uint8)


def planes_to_rgb(ybuf, ubuf, vbuf, shape, y_pitch, y_frame, c_pitch, c_frame, c_step, matrix, y0=0, u0=0, v0=0):
    """Flat uint8 buffers and byte offsets as the header addresses them -> uint8 [Ts,Hs,Ws,3]: the luma of pixel (t, s, x) is
    ybuf[y0 + t * y_frame + s * y_pitch + x], its chroma pair ubuf / vbuf[u0 / v0 + t * c_frame + (s >> 1) * c_pitch +
    (x >> 1) * c_step]."""
    Ts, Hs, Ws = shape
    t, s, x = np.meshgrid(np.arange(Ts), np.arange(Hs), np.arange(Ws), indexing='ij')
    yi = y0 + t * y_frame + s * y_pitch + x
    ci = t * c_frame + (s >> 1) * c_pitch + (x >> 1) * c_step
    return convert(np.asarray(ybuf).reshape(-1)[yi], np.asarray(ubuf).reshape(-1)[u0 + ci], np.asarray(vbuf).reshape(-1)[v0 + ci], matrix)


def clip_to_rgb(y, u, v=None, matrix=PRESETS[('bt601', False)]):
    """Contiguous arrays: y [Ts,Hs,Ws]; I420: u, v [Ts,Hc,Wc]; NV12 (v None): u [Ts,Hc,Wc,2] -> uint8 [Ts,Hs,Ws,3]."""
    y, u = np.ascontiguousarray(y), np.ascontiguousarray(u)
    Ts, Hs, Ws = y.shape
    Hc, Wc = (Hs + 1) // 2, (Ws + 1) // 2
    if v is None:
        assert u.shape == (Ts, Hc, Wc, 2)
        return planes_to_rgb(y, u, u, (Ts, Hs, Ws), Ws, Hs * Ws, 2 * Wc, 2 * Hc * Wc, 2, matrix, v0=1)
    v = np.ascontiguousarray(v)
    assert u.shape == v.shape == (Ts, Hc, Wc)
    return planes_to_rgb(y, u, v, (Ts, Hs, Ws), Ws, Hs * Ws, Wc, Hc * Wc, 1, matrix)


def all_triples():
    """Every (Y, U, V) once -> three int32 arrays of 2^24 entries."""
    i = np.arange(1 << 24, dtype=np.int32)
    return i >> 16, (i >> 8) & 255, i & 255
