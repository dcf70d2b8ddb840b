"""The synthetic inputs of tests/test_gpu_samples_edges.py, made with numpy from fixed seeds. tests/test_samples_edges_host.py reads the
same ones, so what it shows on the CPU holds for the inputs the kernels see. Everything is float32 (uint8 for masks)."""
import zlib

import numpy as np

from distr import fixture

import samples_restatement as sr

MTILE = sr.MTILE
H_B, W_B = 72, 64                                   # point-list and camera cases: 4608 pixels, N valid ones at random positions
NS = (1, 255, 256, 257, 2047, 2048, 2049, 4097)
POINT_CASES = [(sr.SURFACE, 1, N) for N in NS] + [(sr.FREESPACE, number, N) for number in (1, 3, 64) for N in NS]
BATCHES = {'codes_per_view': (4097, 300, 2048), 'empty_view': (257, 0, 2049)}
BIG_HW = (3, 174763)                                # 524 289 pixels, all valid: 257 camera blocks
ONE_HOT_BIG = (0, 2047, 2048, 524287, 524288)
COMPACTION_SIZES = [(1, 1), (23, 89), (32, 64), (3, 683), (1, 524287), (512, 1024), (3, 174763), (17, 61681)]
BELOW_1E5 = np.nextafter(np.float32(1e5), np.float32(0))
SPECIALS = [np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e5, float(BELOW_1E5), 1e-45]
SPECIALS_VALID = [False, False, False, False, False, False, False, True, True]


def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def geometry(H, W):
    """(K_inv, M) as the float32 values the library receives: K_inv = float32(inv(K)) of intrinsic(H, W), M = a rotation times
    a diagonal scale that is not the identity."""
    return np.linalg.inv(intrinsic(H, W)).astype(np.float32), transform().astype(np.float32)


def intrinsic(H, W):
    """fixture.make_intrinsic with the principal point moved out of the image, to (-0.2 W, -0.2 H) (an off-centre crop): h = K_inv (x, y, 1)
    = (x / W + 0.2, y / H + 0.2, 1) then cancels nowhere (off_axis holds at every pixel). With the principal point at the centre, list
    entry 2048 of 4097 valid pixels of a 72-row image always lies next to the principal row."""
    K = fixture.make_intrinsic(H, W)
    K[0, 2], K[1, 2] = -0.2 * W, -0.2 * H
    return K


def transform():
    Q = fixture.make_camera(25.0, -35.0, 1.0, 50.0)[0].astype(np.float64)
    return Q @ np.diag([1.3, 0.8, 1.1])


def cameras(V):
    """RT (V, 3, 4) float32."""
    out = []
    for v in range(V):
        R, T = fixture.make_camera(-50.0 + 45.0 * v, 10.0 + 12.0 * v, 1.5 + 0.1 * v, 8.0 * v + 3.0)
        out.append(np.concatenate([R, T.reshape(3, 1)], 1))
    return np.stack(out).astype(np.float32)


def off_axis(K_inv, pix, W):
    """|h_x|, |h_y| >= 1/16 at this pixel. h = K_inv (x, y, 1) is a difference of two numbers near 1/2: next to the principal point it
    cancels, and the rounding of that one subtraction is no longer small against a sum that holds this pixel ALONE (the one-hot runs;
    at 1/16 it is amplified 8 times, one rounding of the 48 or more the bar counts). Sums over many pixels do not notice."""
    h = np.asarray(K_inv, dtype=np.float64) @ np.array([pix % W, pix // W, 1.0])
    return bool(min(abs(h[0]), abs(h[1])) >= 1.0 / 16)


def depth_with_n_valid(rs, P, N):
    """(P,) float32 with exactly N valid pixels at random positions; the others are 0, -1 or 1e11."""
    d = rs.choice(np.array([0.0, -1.0, 1e11], dtype=np.float32), P)
    at = rs.choice(P, N, replace=False)
    d[at] = rs.uniform(0.8, 2.0, N).astype(np.float32)
    return d


def normals(rs, P):
    n = rs.standard_normal((P, 3))
    return (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)


def draws(rs, mode, number, N):
    """SURFACE: eta (N,) in [0, 0.01); FREESPACE: ratio (number, N) in [0, 1)."""
    if mode == sr.SURFACE:
        return (0.01 * rs.random_sample(N)).astype(np.float32)
    return rs.random_sample((number, N)).astype(np.float32)


def point_case(mode, number, counts):
    """One call of len(counts) views at H_B x W_B: RT (V, 3, 4), depth (V, P), normal (V, P, 3) or None, draws [per view]."""
    P, V = H_B * W_B, len(counts)
    rs = np.random.RandomState(_seed('points', mode, number, tuple(counts)))
    depth = np.stack([depth_with_n_valid(rs, P, n) for n in counts])
    normal = np.stack([normals(rs, P) for _ in counts]) if mode == sr.SURFACE else None
    return dict(RT=cameras(V), depth=depth, normal=normal, draws=[draws(rs, mode, number, n) for n in counts])


def big_case():
    """FREESPACE, number 1, one view of BIG_HW, every pixel valid."""
    rs = np.random.RandomState(_seed('big'))
    P = BIG_HW[0] * BIG_HW[1]
    return dict(RT=cameras(1), depth=rs.uniform(0.8, 2.0, (1, P)).astype(np.float32), normal=None, draws=[draws(rs, sr.FREESPACE, 1, P)])


def upstream(key, n):
    """n values, uniform in +-[0.5, 1.5], float32."""
    rs = np.random.RandomState(_seed('upstream', key))
    return (rs.uniform(0.5, 1.5, n) * rs.choice([-1.0, 1.0], n)).astype(np.float32)


def block_edges(P):
    """Pixels b 2048 - 1 and b 2048 for every b, inside the image."""
    b = np.arange(0, P + MTILE, MTILE)
    e = np.concatenate([b - 1, b])
    return np.unique(e[(e >= 0) & (e < P)])


PATTERNS = ('all', 'none', 'last', 'edges', 'half', 'specials')


def valid_pattern(name, P):
    """(P,) bool: which pixels are valid. 'specials' is 'half' here; depth_pattern overwrites the block edges."""
    rs = np.random.RandomState(_seed('pattern', name, P))
    on = np.zeros(P, dtype=bool)
    if name == 'all':
        on[:] = True
    elif name == 'last':
        on[P - 1] = True
    elif name == 'edges':
        on[block_edges(P)] = True
    elif name in ('half', 'specials'):
        on = rs.random_sample(P) < 0.5
    return on


def depth_pattern(name, P):
    """(P,) float32 depth map of the pattern: valid pixels in [0.5, 3), the others 0, -1 or 1e11; 'specials' puts NaN, +-inf, -1, 0, -0.0,
    1e5, the float below 1e5 and a subnormal on and next to the block boundaries, cycling."""
    rs = np.random.RandomState(_seed('depth', name, P))
    on = valid_pattern(name, P)
    d = np.where(on, rs.uniform(0.5, 3.0, P), rs.choice([0.0, -1.0, 1e11], P)).astype(np.float32)
    if name == 'specials':
        e = block_edges(P)
        at = np.unique(np.concatenate([e, e[e + 1 < P] + 1]))
        j = np.arange(at.size)                      # 27 consecutive positions hold every special before, on and behind a boundary
        d[at] = np.array(SPECIALS, dtype=np.float32)[(j + j // len(SPECIALS) + P) % len(SPECIALS)]
    return d


def mask_pattern(name, P):
    """(P,) uint8 mask of the pattern: 0 off, 1 or 255 on ('specials': 255 and 1 alternate on the block boundaries, 0 next to them)."""
    rs = np.random.RandomState(_seed('mask', name, P))
    m = np.where(valid_pattern(name, P), rs.choice(np.array([1, 255], dtype=np.uint8), P), 0).astype(np.uint8)
    if name == 'specials':
        e = block_edges(P)
        m[e] = np.where(np.arange(e.size) % 2, 1, 255).astype(np.uint8)
        nxt = e[e + 1 < P] + 1
        m[nxt[~np.isin(nxt, e)]] = 0
    return m


def call_patterns(call):
    """The three patterns of compaction call 0, 1, 2: every pattern appears, in changing view slots."""
    return [PATTERNS[(2 * call + v) % len(PATTERNS)] for v in range(3)]
