"""The render backward's bookkeeping at its edges: the sample list (k_bwd_prep count / k_bwd_scan / k_bwd_prep emit), its cut into
64- and 32-sample tiles (bwd_range, the two launch_bwd grids), the views of a batch (vprefix / vfind), the chunks of 64 partial rows
(k_bwd_reduce, k_bwd_final) and the appended pad sample.

The device: a pixel inside the sphere whose only upstream gradient is g_min_sdf != 0 emits exactly one sample (row k = 0, coefficient
g_min_sdf), and with only such pixels the list is in ascending pixel order. A case of count N is N chosen pixels: a few HEAVY ones
(distinct coefficients of order 1) at the list positions bwd_list_restatement.edge_positions names -- position 0, N - 1, the first
sample of the last tile, both sides of the hand-over between the two kernels, the first sample of every 64th partial row -- among
fillers of +-2^-40, which fix the list's length and layout. Losing, doubling or mis-associating one heavy sample is an error of order 1.

Expected values: g_latent = sum over the CPU oracle's sample list of coef x (float64 code gradient at the sample's point), on the oracle's
ReLU pattern for every sample of order 1 and on float64's own for the fillers (their contribution is part of the sum, not neglected);
g_R, g_T from the oracle's backward of the same upstream gradient. Bar: 1e-4 of the expected tensor's largest entry, the project's bar
for a different f32 summation order; where the expected tensor is all zero the kernel's is too. Every call runs on a backward workspace
of exactly nviews x bwd_bytes, filled with 0xFF (a stale partial or chunk row reads as NaN, a stale offset as -1) between two 4 KiB
guards of 0xA5, on one saved forward per engine and scene. The observed residuals are recorded in DESIGN.md section 5."""
import ctypes as C
import os

import numpy as np
import pytest

import bwd_list_restatement as bl

pytestmark = pytest.mark.gpu

BAR = 1e-4
GUARD = 4096
FILL = np.float32(2.0 ** -40)
HEAVY = np.array([1.0, -0.75, 0.5, -0.875, 0.625, -0.9375, 0.6875, -0.5625, 0.8125, -0.4375, 0.59375, -0.65625, 0.78125, -0.71875,
                  0.53125, -0.96875], np.float32)

KW_A = dict(marcher='recursive', march_step=30, buffer_size=2, want_normal=False)
KW_C = dict(marcher='recursive', march_step=30, buffer_size=8, clamp_dist=1.0, want_normal=False)
CAMERA_A = (20, 10, 1.6, 0)

COUNTS_SPLIT = (1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4096, 4097, 8191, 8192, 8193, 12288, 12289, 16383, 16384, 16385, 16416, 16417,
                24575, 24576, 24577, 25600)
COUNTS_FULL = (1, 63, 64, 65, 4096, 4097, 16384, 16385)
PREFIX_COUNTS = (12289, 25600)                       # these take the pixels 0 .. N - 1, every other count a seeded random subset
BATCH_COUNTS = (0, 1, 65, 16385, 33, 8193, 64, 24577)


# ------------------------------------------------------------------------------------------------ the CPU side: scenes and expected values
def oracle_gates(O, Ws, latent, pts):
    """The oracle's ReLU pattern at `pts` (the f32 kernel's: the decoder tile is bit-identical to it), eight boolean arrays. The oracle
    evaluates one layer of one point list per call, serially and outside the GIL: the calls run side by side."""
    from concurrent.futures import ThreadPoolExecutor
    cuts = [0, len(pts)] if len(pts) <= 1024 else [0, len(pts) // 2, len(pts)]
    with ThreadPoolExecutor(16) as pool:
        parts = [[pool.submit(O.layer_activations, latent, pts[a:b], l) for a, b in zip(cuts[:-1], cuts[1:])] for l in range(8)]
        return [np.concatenate([f.result() for f in fs])[:, :Ws[l].shape[0]] > 0 for l, fs in enumerate(parts)]


class Scene(object):
    """One oracle render and, per pixel inside the sphere, the point of its row k = 0 and the float64 code gradient there."""

    def __init__(self, O, orc, decoder, H, R, T, kw):
        from distr import fixture
        self.O, (self.Ws, self.bs, self.latent) = O, decoder
        self.H, self.P, self.K, self.R, self.T, self.kw = H, H * H, fixture.make_intrinsic(H, H), np.asarray(R, np.float32), np.asarray(T, np.float32), kw
        out = O.render(orc.make_cfg(H, H, self.K, **kw), self.latent, self.R, self.T)
        self.state, self.mask = out['state'], out['mask'].astype(bool)
        pix, pts, coef = self.state.samples(g_min_sdf=np.ones(self.P, np.float32))
        assert (pix >= 0).all() and (np.diff(pix) > 0).all() and (coef == 1).all()       # one sample per pixel, ascending, no pad
        self.pix, self.pts = pix.astype(np.int64), pts
        self.row = np.full(self.P, -1, np.int64)
        self.row[self.pix] = np.arange(len(self.pix))
        self._U, self._gated = None, {}

    @property
    def U(self):
        if self._U is None:
            self._U = bl.unit_code_gradients(self.Ws, self.bs, self.latent, self.pts)
        return self._U

    def gated_rows(self, pts):
        """Float64 code gradients at `pts` on the oracle's ReLU pattern."""
        return bl.unit_code_gradients(self.Ws, self.bs, self.latent, pts, oracle_gates(self.O, self.Ws, self.latent, pts))

    def expected_min_sdf(self, g, heavy):
        """(g_latent (256,), g_R (3, 3), g_T (3,), samples) for the upstream gradient g on min_sdf alone."""
        new = [int(p) for p in heavy if int(p) not in self._gated]
        if new:
            for p, r in zip(new, self.gated_rows(self.pts[self.row[new]])):
                self._gated[p] = r
        coef = g[self.pix].astype(np.float64)
        sel = np.flatnonzero(coef)
        e = coef[sel] @ self.U[sel]
        for p in heavy:
            e += float(g[p]) * (self._gated[int(p)] - self.U[self.row[p]])
        _, gR, gT, ns = self.state.backward(g_min_sdf=g)
        assert ns == len(sel)
        return e, gR.astype(np.float64), gT.astype(np.float64), ns


@pytest.fixture(scope='module')
def scene_a(cpu_oracle, orc, fixture_decoder):
    from distr import fixture
    s = Scene(cpu_oracle, orc, fixture_decoder, 160, *fixture.make_camera(*CAMERA_A), kw=KW_A)
    assert len(s.pix) == s.P == 25600 and int(s.mask.sum()) == 5716          # the whole image lies inside the sphere's outline
    return s


def case_gradient(scene, n, split, seed, prefix=False):
    """g_min_sdf of a case of count n: fillers on n pixels, heavy coefficients at the edge positions of its tile plan."""
    rs = np.random.RandomState(seed)
    chosen = scene.pix[:n] if prefix else np.sort(rs.choice(scene.pix, n, replace=False))
    g = np.zeros(scene.P, np.float32)
    g[chosen] = rs.choice([-FILL, FILL], n)
    pos = bl.edge_positions(n, split)
    assert len(pos) <= len(HEAVY)
    heavy = chosen[pos]
    g[heavy] = HEAVY[:len(pos)]
    return g, heavy


# ------------------------------------------------------------------------------------------------ the GPU side: one forward, many backwards
def _engine(fixture_decoder, **env):
    """A context of its own created under `env` (the DISTR_* knobs are read by distr_create)."""
    from distr import functions
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return functions.engine_from_weights(fixture_decoder[0], fixture_decoder[1], 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Forward(object):
    """render_batch_call of B views with codes and cameras that require grad; backward() calls distr_render_backward_batch on the
    saved forward workspace as RenderBatchFunction.backward does, on a workspace this class owns."""

    def __init__(self, eng, latent, H, K, Rs, Ts, kw):
        import torch
        from distr import binding, functions
        dev = eng.device
        self.eng, self.B, self.P = eng, len(Rs), H * H
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev).requires_grad_(True)
        self.inputs = (t(np.repeat(latent, self.B, 0)), t(np.stack(Rs)), t(np.stack(Ts)))
        self.out = functions.render_batch_call(eng, binding.make_cfg((H, H), K, arith='f32', **kw), *self.inputs)
        self.node = self.out[2].grad_fn
        self.bytes = self.B * eng.ctx.workspace_bytes(self.node.cfg)[1]
        self.buf = torch.empty(self.bytes + 2 * GUARD, dtype=torch.uint8, device=dev)

    def backward(self, g_min_sdf=None, g_zdepth=None):
        """-> (g_latent (B, 256), g_R (B, 3, 3), g_T (B, 3)) float64, per-view num_grad_samples. Asserts finite outputs and whole guards."""
        import torch
        from distr import binding
        eng, node, B, n = self.eng, self.node, self.B, self.bytes
        dev = eng.device
        self.buf[:GUARD] = 0xA5
        self.buf[GUARD:GUARD + n] = 0xFF
        self.buf[GUARD + n:] = 0xA5
        ws_b = self.buf[GUARD:GUARD + n]
        up = lambda g: None if g is None else torch.from_numpy(np.ascontiguousarray(g, np.float32).reshape(B, self.P)).to(dev)
        gq, gz = up(g_min_sdf), up(g_zdepth)
        nan = lambda *s: torch.full(s, float('nan'), dtype=torch.float32, device=dev)
        g_lat, g_R, g_T = nan(B, eng.latent_size), nan(B, 9), nan(B, 3)
        p = binding.ptr
        eng.ctx.check(eng.ctx.L.distr_render_backward_batch(
            eng.ctx.h, C.byref(node.cfg), B, p(node.ws), node.ws.numel(), p(gz), p(gq), None, None, p(g_lat), p(g_R), p(g_T),
            p(ws_b), n, eng.ctx.stream()))
        torch.cuda.synchronize()
        counts = [int(eng.ctx.render_stats(node.cfg, node.ws[v * node.view_bytes:])['num_grad_samples']) for v in range(B)]
        assert bool((self.buf[:GUARD] == 0xA5).all()) and bool((self.buf[GUARD + n:] == 0xA5).all()), 'a guard of the backward workspace was written'
        got = g_lat.double().cpu().numpy(), g_R.double().cpu().numpy().reshape(B, 3, 3), g_T.double().cpu().numpy()
        assert all(np.isfinite(a).all() for a in got), ('non-finite gradient', counts)
        return got, counts


def _forward_a(eng, scene, B=1):
    return Forward(eng, scene.latent, scene.H, scene.K, [scene.R] * B, [scene.T] * B, scene.kw)


@pytest.fixture(scope='module')
def fwd_split(engine, scene_a):
    return _forward_a(engine, scene_a)


@pytest.fixture(scope='module')
def fwd_full(fixture_decoder, scene_a):
    return _forward_a(_engine(fixture_decoder, DISTR_SAVE_MASKS=0), scene_a)


def check(label, got, exp):
    """got, exp: (g_latent, g_R, g_T) of one view. Prints the residuals (of the expected tensor's largest entry), asserts the bar."""
    res = []
    for name, a, b in zip(('g_latent', 'g_R', 'g_T'), got, exp):
        a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
        if not b.any():
            assert not a.any(), (label, name, 'expected all zero', float(np.abs(a).max()))
            res.append(0.0)
        else:
            res.append(float(np.abs(a - b).max() / np.abs(b).max()))
    print('%s: residuals g_latent %.3e g_R %.3e g_T %.3e' % ((label,) + tuple(res)))
    assert max(res) <= BAR, (label, res)
    return res


def _run_count(scene, fwd, n, split):
    g, heavy = case_gradient(scene, n, split, 1000 + n, prefix=n in PREFIX_COUNTS)
    exp = scene.expected_min_sdf(g, heavy)
    got, counts = fwd.backward(g_min_sdf=g)
    assert counts == [n] and exp[3] == n, (counts, exp[3], n)
    check('%s list, %d samples (%d heavy)' % ('split' if split else 'unsplit', n, len(heavy)), [a[0] for a in got], exp[:3])


def _run_empty(scene, fwd, split, full):
    """A full list, then an empty one on the same workspace: all three gradients exactly zero, nothing left of the call before."""
    _run_count(scene, fwd, full, split)
    got, counts = fwd.backward(g_min_sdf=np.zeros(scene.P, np.float32))
    assert counts == [0]
    assert not any(a.any() for a in got), [float(np.abs(a).max()) for a in got]
    _, gR, gT, ns = scene.state.backward(g_min_sdf=np.zeros(scene.P, np.float32))
    assert ns == 0 and not gR.any() and not gT.any()


# ------------------------------------------------------------------------------------------------ 1, 2: one view, the counts at every edge
@pytest.mark.parametrize('n', COUNTS_SPLIT)
def test_split_list_counts(scene_a, fwd_split, n):
    """The default engine (masks saved, the list split by bwd_range): 32-sample tiles and their chunk edges (64 / 65, 128 / 129 rows), the
    switch to 64-sample tiles above a remainder of 8 192, a whole round with no remainder, with one sample, with one and two 32-sample
    tiles behind it, the second switch at 16 384 + 8 192, the whole image."""
    _run_count(scene_a, fwd_split, n, True)


def test_split_list_empty_after_full(scene_a, fwd_split):
    _run_empty(scene_a, fwd_split, True, 25600)


@pytest.mark.parametrize('n', COUNTS_FULL)
def test_unsplit_list_counts(scene_a, fwd_full, n):
    """An engine created under DISTR_SAVE_MASKS=0 (k_bwd<BWD_FULL>: 64-sample tiles throughout, no split)."""
    _run_count(scene_a, fwd_full, n, False)


def test_unsplit_list_empty_after_full(scene_a, fwd_full):
    _run_empty(scene_a, fwd_full, False, 16385)


# ------------------------------------------------------------------------------------------------ 3: the views of a batch
@pytest.fixture(scope='module')
def batch(engine, scene_a, fwd_split):
    """One forward of 8 views of scene A; per view a pixel subset of its own; the stand-alone gradients of every view."""
    fwd = _forward_a(engine, scene_a, len(BATCH_COUNTS))
    G = np.stack([case_gradient(scene_a, n, True, 2000 + v)[0] for v, n in enumerate(BATCH_COUNTS)])
    alone = []
    for v, n in enumerate(BATCH_COUNTS):
        got, counts = fwd_split.backward(g_min_sdf=G[v])
        assert counts == [n]
        alone.append([a[0] for a in got])
    return fwd, G, alone


@pytest.mark.parametrize('order', ['as listed', 'reversed'])
def test_batch_views_equal_their_own_call(batch, order):
    """One backward call over 8 views with the counts [0, 1, 65, 16385, 33, 8193, 64, 24577] (and reversed: vfind walks the
    concatenation of the views' tiles): every view's sample count is its own and its g_latent, g_R, g_T are, byte for byte, those of
    the stand-alone call of that view."""
    fwd, G, alone = batch
    idx = list(range(len(BATCH_COUNTS)))
    if order == 'reversed':
        idx = idx[::-1]
    got, counts = fwd.backward(g_min_sdf=G[idx])
    assert counts == [BATCH_COUNTS[i] for i in idx], counts
    for v, i in enumerate(idx):
        for name, a, b in zip(('g_latent', 'g_R', 'g_T'), got, alone[i]):
            assert np.array_equal(a[v], b), (order, 'view %d (count %d)' % (v, BATCH_COUNTS[i]), name, float(np.abs(a[v] - b).max()))
        if BATCH_COUNTS[i] == 0:
            assert not any(a[v].any() for a in got)


# ------------------------------------------------------------------------------------------------ 4: the ragged end of the scan
SCAN_H = 264                                             # P = 69 696: 273 blocks of 256 pixels, k_bwd_scan walks 2 per thread, thread 136 one
SCAN_T = ((1.4, 1.4, 3.0), (-1.4, -1.4, 3.0))            # samples in the blocks 173 .. 272 (last pixel P - 1) / in the blocks 0 .. 100


@pytest.fixture(scope='module')
def scan_scenes(cpu_oracle, orc, fixture_decoder):
    return [Scene(cpu_oracle, orc, fixture_decoder, SCAN_H, np.eye(3), T, KW_A) for T in SCAN_T]


def _scan_gradient(scene, seed):
    """Every pixel inside the sphere; heavy: the first and the last sample, the first sample behind every run of empty blocks, the last
    sample of block 2t and the first of block 2t + 1 of one populated pair (one thread of k_bwd_scan), the edge positions of the tile plan."""
    rs = np.random.RandomState(seed)
    pix = scene.pix
    n = len(pix)
    blk = pix // bl.PREP_BLOCK
    per, own = bl.scan_plan((scene.P + bl.PREP_BLOCK - 1) // bl.PREP_BLOCK)
    assert per == 2 and own[-1][2] - own[-1][1] == 1
    pos = set(bl.edge_positions(n, True))
    pos.update(int(i) for i in np.flatnonzero(np.diff(blk) > 1) + 1)
    pos.add(0)
    pairs = [t for t, b0, b1 in own if b1 - b0 == 2 and (blk == b0).any() and (blk == b0 + 1).any()]
    t = pairs[len(pairs) // 2]
    pos.update((int(np.flatnonzero(blk == 2 * t)[-1]), int(np.flatnonzero(blk == 2 * t + 1)[0])))
    pos = sorted(pos)
    g = np.zeros(scene.P, np.float32)
    g[pix] = rs.choice([-FILL, FILL], n)
    assert len(pos) <= len(HEAVY)
    g[pix[pos]] = HEAVY[:len(pos)]
    return g, pix[pos]


def test_scan_ragged_end(engine, scan_scenes):
    """nblk = 273 is no multiple of k_bwd_scan's 256 threads: two blocks per thread and a last thread with one. View 0's samples lie in the
    blocks 173 .. 272 behind 173 empty ones and end on pixel P - 1 in the lone block of thread 136; view 1 (the mirrored camera) starts
    on pixel 0 in block 0 and leaves the blocks behind 100 empty."""
    a, b = scan_scenes
    assert len(a.pix) == 7997 and int(a.mask.sum()) == 1654 and a.pix[0] == 44328 and a.pix[-1] == a.P - 1
    assert len(np.unique(a.pix // 256)) == 100 and a.pix[0] // 256 == 173
    assert b.pix[0] == 0 and b.pix[-1] // 256 < 272
    fwd = Forward(engine, a.latent, SCAN_H, a.K, [a.R, b.R], [a.T, b.T], KW_A)
    gs = [_scan_gradient(s, 3000 + v) for v, s in enumerate((a, b))]
    got, counts = fwd.backward(g_min_sdf=np.stack([g for g, _ in gs]))
    assert counts == [len(a.pix), len(b.pix)], counts
    for v, s in enumerate((a, b)):
        exp = s.expected_min_sdf(*gs[v])
        check('scan scene view %d, %d samples (%d heavy)' % (v, exp[3], len(gs[v][1])), [x[v] for x in got], exp[:3])


# ------------------------------------------------------------------------------------------------ 5: the pad sample
def _pad_case(O, orc, decoder, H, target):
    """Scene C at H x H: a g_zdepth on hit pixels whose list ends with the combined pad sample, topped up with g_min_sdf-only pixels (one
    sample each) to exactly `target` real samples. Returns (scene data, g_zdepth, g_min_sdf, the oracle's list)."""
    from distr import fixture
    Ws, bs, latent = decoder
    K = fixture.make_intrinsic(H, H)
    R, T = fixture.make_camera(*CAMERA_A)
    out = O.render(orc.make_cfg(H, H, K, **KW_C), latent, R, T)
    st, P = out['state'], H * H
    hits = np.flatnonzero(out['mask'])
    gz = np.zeros(P, np.float32)
    gz[hits] = 1
    pix, _, _ = st.samples(g_zdepth=gz)
    assert pix[-1] == -1 and (pix[:-1] >= 0).all()
    rows = np.bincount(pix[:-1], minlength=P)                      # real rows per hit pixel; a pixel with fewer than 8 has padded rows
    if rows.sum() <= target:
        S = hits
    else:
        short = hits[rows[hits] < KW_C['buffer_size']][0]
        S = np.concatenate([[short], hits[hits != short][:6]])
    rs = np.random.RandomState(4000 + H)
    gz[:] = 0
    gz[S] = rs.uniform(0.5, 1.0, len(S))                           # one sign: the pad rows' coefficients cannot cancel
    top = target - int(rows[S].sum())
    free = np.setdiff1d(np.flatnonzero(~out['mask'].astype(bool)), S)
    assert 0 <= top <= len(free), (top, len(free))
    gq = np.zeros(P, np.float32)
    T_px = rs.choice(free, top, replace=False)
    gq[T_px] = rs.uniform(0.5, 1.0, top) * rs.choice([-1.0, 1.0], top)
    lst = st.samples(g_zdepth=gz, g_min_sdf=gq)
    assert len(lst[0]) == target + 1 and lst[0][-1] == -1 and (lst[0][:-1] >= 0).all() and lst[2][-1] != 0, (len(lst[0]), lst[0][-3:], lst[2][-3:])
    return dict(H=H, K=K, R=R, T=T, latent=latent, state=st), gz, gq, lst


@pytest.mark.parametrize('H,target', [(32, 64), (64, 8192)])
def test_pad_sample_at_a_tile_edge(engine, cpu_oracle, orc, fixture_decoder, H, target):
    """clamp_dist = 1.0 lets the padded rows of a short ray carry a coefficient: k_bwd_scan appends one combined sample behind the list.
    With 64 real samples it is list entry 64, alone in the third 32-sample tile; with 8 192 it makes the count 8 193 and flips the whole
    list to 64-sample tiles. Expected values from the oracle's full list, every sample on the oracle's ReLU pattern."""
    Ws, bs, latent = fixture_decoder
    c, gz, gq, (pix, pts, coef) = _pad_case(cpu_oracle, orc, fixture_decoder, H, target)
    plan = bl.tile_plan(target + 1, True)
    assert plan['per_kernel'] == ({64: 0, 32: 3} if target == 64 else {64: 129, 32: 0})
    e = coef.astype(np.float64) @ bl.unit_code_gradients(Ws, bs, latent, pts, oracle_gates(cpu_oracle, Ws, latent, pts))
    _, gR, gT, ns = c['state'].backward(g_zdepth=gz, g_min_sdf=gq)
    assert ns == target + 1
    fwd = Forward(engine, latent, H, c['K'], [c['R']], [c['T']], KW_C)
    got, counts = fwd.backward(g_min_sdf=gq, g_zdepth=gz)
    assert counts == [target + 1], counts
    check('pad scene %d x %d, %d real samples + pad (coefficient %g)' % (H, H, target, coef[-1]), [a[0] for a in got], (e, gR, gT))
