"""The dropout mask of the layer-wise train path, restated in numpy from its definition -- not from the kernel:

    keep(seed, l, g, i, n) = out[i & 3] >= T
      out = philox4x32_10(counter = (i >> 2, g, n, l), key = (seed & 0xffffffff, seed >> 32))
      T     = min(2^32 - 1, floor(p * 2^32))
      scale = float32(1 / (1 - p))

l: the layer whose relu output is dropped, n: its output unit, g: the segment's global index, i: the point's index inside its segment.
Philox4x32-10 with the Random123 constants. Everything is vectorised over uint64 arrays that hold 32-bit words.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LOW = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, broadcast against each other; key: two ints. Returns four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & LOW for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in counter])]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]           # 32 x 32 -> 64 bit products: no overflow in uint64
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & LOW, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & LOW]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def threshold(p):
    return min((1 << 32) - 1, int(np.floor(np.float64(p) * np.float64(4294967296.0))))


def scale(p):
    return float(np.float32(1.0 / (1.0 - np.float64(p))))


def keep_at(seed, T, layer, segment, point, unit):
    """keep for arrays (or ints) of layers, global segment indices, points in segment and units, broadcast against each other: bool."""
    layer, segment, point, unit = np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in (layer, segment, point, unit)])
    out = philox4x32_10((point >> np.uint64(2), segment, unit, layer), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))
    lane = point & np.uint64(3)
    draw = np.where(lane == 0, out[0], np.where(lane == 1, out[1], np.where(lane == 2, out[2], out[3])))
    return draw >= np.uint32(T)


def keep(seed, layer, segment, npoints, nunits, T):
    """(npoints, nunits) bool: the mask of lin_layer's output for the first npoints points of global segment `segment`."""
    return keep_at(seed, T, layer, segment, np.arange(npoints, dtype=np.uint64)[:, None], np.arange(nunits, dtype=np.uint64)[None, :])


def keep_list(seed, layer, counts, nunits, T, segment_base=0):
    """(sum counts, nunits) bool for a segmented point list: segment s has the global index segment_base + s."""
    parts = [keep(seed, layer, segment_base + s, int(n), nunits, T) for s, n in enumerate(counts)]
    return np.concatenate(parts, 0) if parts else np.zeros((0, nunits), dtype=bool)


def g32_bits(golden, case, kind, layer, rows=210, latent_size=256):
    """Golden G32 (tests/gen_golden_train_forward.py): the (rows, units) bool array `kind` ('pos', 'near', 'keep') of lin_layer's output."""
    if layer == 3:
        packed, units = golden['%s_%s3' % (case, kind)], 509 - latent_size
    else:
        packed, units = golden['%s_%s' % (case, kind)][layer if layer < 3 else layer - 1], 512
    return np.unpackbits(packed)[:rows * units].reshape(rows, units).astype(bool)
