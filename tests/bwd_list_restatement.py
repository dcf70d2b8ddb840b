"""Python restatement of how the render backward cuts a view's gradient-sample list into tiles, partial rows and reduction chunks, and a
float64 code gradient per sample, for tests/test_gpu_bwd_list.py and tests/test_bwd_list_host.py. No GPU.

tile_plan() is used to AIM a test (which list positions sit at a tile, round or chunk edge); it is never an expected value. The
expected values are float64 sums over the CPU oracle's sample list (unit_code_gradients below, the oracle's own backward for the
camera)."""
import numpy as np

# The constants below restate the native code; tests/test_bwd_list_host.py checks that the plan they give is consistent with itself and
# with the sizes the host allocates and launches.
ROUND = 16384        # csrc/distr_kernels.hpp, bwd_range: `full = (count / 16384) * 16384` -- whole rounds of 256 tiles x 64 samples
REM_MAX = 8192       # bwd_range: `if (!split || rem > 8192)` -- the largest remainder that goes to 32-sample tiles
TILE_BIG = 64        # k_bwd<.., RB = 2>: TILE = 32 * RB; render_backward_impl: `constexpr int TILE = 64`
TILE_SMALL = 32      # k_bwd<.., RB = 1>
BWD_CHUNK = 64       # csrc/distr_api.hip: `constexpr int BWD_CHUNK = 64` -- partial rows per k_bwd_reduce chunk
PREP_BLOCK = 256     # k_bwd_prep: `px = blockIdx.x * 256 + threadIdx.x`; render_backward_impl: `nblk = (P + 255) / 256`
SCAN_THREADS = 256   # k_bwd_scan: `per = (nblk + 255) / 256`, one block of 256 threads per view


def bwd_range(count, split, tile_size):
    """bwd_range of csrc/distr_kernels.hpp: (lo, hi, first_tile, ntiles) of the kernel with `tile_size`-sample tiles."""
    count = int(count)
    full = (count // ROUND) * ROUND
    rem = count - full
    if not split or rem > REM_MAX:
        hi = count if (tile_size == TILE_BIG or not split) else 0
        ntiles = (count + tile_size - 1) // tile_size
        if split:
            ntiles = (count + 63) // 64
        return 0, hi, 0, ntiles
    t64 = full // 64
    ntiles = t64 + (rem + 31) // 32
    if tile_size == TILE_BIG:
        return 0, full, 0, ntiles
    return full, count, t64, ntiles


def prows(smax):
    """render_backward_impl: `prows = (smax + 31) / 32 + 256`, the partial rows it carves (bwd_bytes sizes the same)."""
    return (int(smax) + 31) // 32 + 256


def launch_grids(smax, split):
    """Workgroups per view of the launch_bwd calls of render_backward_impl: {tile size: grid}. Split (saved masks): `(smax + 63) / 64`
    for the 64-sample kernel and `(min(smax, 8192) + 31) / 32` for the 32-sample one; unsplit: `tiles = (smax + 63) / 64`."""
    smax = int(smax)
    if not split:
        return {TILE_BIG: (smax + 63) // 64}
    return {TILE_BIG: (smax + 63) // 64, TILE_SMALL: (min(smax, REM_MAX) + 31) // 32}


def tile_plan(count, split):
    """The tiles of a list of `count` samples as k_bwd walks them (split: the engine saves masks; unsplit: DISTR_SAVE_MASKS=0).
    Returns a dict: row / lo / hi / size -- int64 arrays, one entry per tile in partial-row order: the tile's partial row, its list
    range [lo, hi) and its tile size; ntiles (partial rows k_bwd_reduce sums), nchunks (chunks k_bwd_final sums), full (end of the
    64-sample kernel's range), per_kernel {tile size: number of its tiles}."""
    count = int(count)
    rows, los, his, sizes, per_kernel = [], [], [], [], {}
    ntiles = 0
    for ts in ((TILE_BIG, TILE_SMALL) if split else (TILE_BIG,)):
        lo, hi, first, ntiles = bwd_range(count, split, ts)
        n = (hi - lo + ts - 1) // ts                # k_bwd: `mine = (hi - lo + TILE - 1) / TILE`
        per_kernel[ts] = n
        local = np.arange(n, dtype=np.int64)
        rows.append(first + local)                  # `tile = first + local`
        los.append(lo + local * ts)                 # `base = lo + local * TILE`
        his.append(np.minimum(lo + (local + 1) * ts, hi))
        sizes.append(np.full(n, ts, np.int64))
    full = bwd_range(count, split, TILE_BIG)[1]
    return dict(row=np.concatenate(rows), lo=np.concatenate(los), hi=np.concatenate(his), size=np.concatenate(sizes), ntiles=int(ntiles),
                nchunks=(int(ntiles) + BWD_CHUNK - 1) // BWD_CHUNK, full=int(full), per_kernel=per_kernel)


def edge_positions(count, split):
    """The list positions a case of `count` samples makes heavy: position 0, count - 1, the first sample of the last tile, both sides
    of the hand-over between the 64- and the 32-sample kernel, the first sample of partial row 64 and of every later multiple of 64."""
    count = int(count)
    if count == 0:
        return []
    plan = tile_plan(count, split)
    order = np.argsort(plan['row'])
    lo = plan['lo'][order]
    pos = {0, count - 1, int(lo[-1])}
    if 0 < plan['full'] < count:
        pos.update((plan['full'] - 1, plan['full']))
    pos.update(int(lo[r]) for r in range(BWD_CHUNK, plan['ntiles'], BWD_CHUNK))
    return sorted(pos)


def scan_plan(nblk):
    """k_bwd_scan: thread t owns the 256-pixel blocks [b0, b1) -- `per = (nblk + 255) / 256; b0 = t * per; b1 = min(nblk, b0 + per)`.
    Returns (per, [(t, b0, b1) for the threads that own a block])."""
    per = (int(nblk) + SCAN_THREADS - 1) // SCAN_THREADS
    own = [(t, t * per, min(nblk, t * per + per)) for t in range(SCAN_THREADS) if t * per < nblk]
    return per, own


def unit_code_gradients(Ws, bs, latent, pts, gates=None, chunk=2048):
    """Row i: d sdf(latent, pts[i]) / d latent in float64, the ReLUs of layer l being gates[l] (own pattern: None) -- what
    train_restatement.gradients(Ws, bs, codes, pts, [1] * n, ones, gates=gates)[4] returns, without the weight gradients (only the
    code rows require grad, so autograd never forms them) and in chunks of `chunk` samples."""
    import torch
    import train_restatement as tr
    W64, b64 = tr.to64(Ws), tr.to64(bs)
    lat, = tr.to64([np.asarray(latent).reshape(1, -1)])
    p64, = tr.to64([np.asarray(pts).reshape(-1, 3)])
    out = np.zeros((p64.shape[0], lat.shape[1]))
    for i0 in range(0, p64.shape[0], chunk):
        i1 = min(p64.shape[0], i0 + chunk)
        codes = lat.repeat(i1 - i0, 1).requires_grad_(True)
        g = None if gates is None else [torch.as_tensor(np.asarray(m))[i0:i1] for m in gates]
        y, _ = tr.forward(W64, b64, codes, p64[i0:i1], [1] * (i1 - i0), None, g)
        y.sum().backward()
        out[i0:i1] = codes.grad.numpy()
    return out
