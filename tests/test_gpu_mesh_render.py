"""Depth, normal and mask maps of a triangle mesh on the GPU (include/distr_mesh.h: distr_mesh_render; distr/mesh.py: render_mesh;
SDFRenderer.render_mesh): every output bit for bit against the numpy float32 restatement (tests/mesh_render_restatement.py, validated
on the CPU by tests/test_mesh_render_host.py) at the tile, chunk and block edges; determinism and independence of the views, the skip
rules, the winding; the renderer's method against the function; the maps against the sphere tracer on the fixture decoder's own
marching-cubes mesh; and the maps fed to SDFRenderer_deepsdf.get_samples."""
import functools

import numpy as np
import pytest

import mesh_render_restatement as Q
import mesh_restatement as R
import mesh_sdf_restatement as S

pytestmark = pytest.mark.gpu
TILE, CH = Q.RENDER_TILE, Q.RENDER_CHUNK
KEYS = ('depth', 'normal', 'mask', 'zdepth', 'face', 'bary')
M64 = Q.M_DEFAULT.astype(np.float64)


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _render(v, f, K, RT, hw, M=None, frame='image'):
    """distr.mesh.render_mesh with details -> dict of numpy arrays; shapes and dtypes checked."""
    import torch
    from distr import mesh
    out = mesh.render_mesh(_cuda(v), _cuda(f), K, _cuda(RT), hw, transform_matrix=M, normal_frame=frame, details=True)
    lead = tuple(np.shape(RT)[:-2])
    want = {'depth': (torch.float32, ()), 'normal': (torch.float32, (3,)), 'mask': (torch.uint8, ()), 'zdepth': (torch.float32, ()),
            'face': (torch.int64, ()), 'bary': (torch.float32, (2,))}
    for k, o in zip(KEYS, out):
        assert o.dtype == want[k][0] and tuple(o.shape) == lead + tuple(hw) + want[k][1], (k, o.dtype, o.shape)
    return {k: o.cpu().numpy() for k, o in zip(KEYS, out)}


def _same_bytes(a, b, keys=KEYS):
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _equals_restatement(got, want):
    """mask and face equal; depth, zdepth, bary and the normals bit for bit."""
    assert np.array_equal(got['mask'], want['mask']), int((got['mask'] != want['mask']).sum())
    assert np.array_equal(got['face'], want['face']), int((got['face'] != want['face']).sum())
    for k in ('depth', 'zdepth', 'bary', 'normal'):
        a, b = got[k].view(np.uint32), np.ascontiguousarray(want[k], np.float32).view(np.uint32)
        assert np.array_equal(a, b), (k, int((a != b).sum()), float(np.abs(got[k] - want[k]).max()))


# ------------------------------------------------------------------------------------------------------- random soups
@functools.lru_cache(maxsize=None)
def _soup(nf):
    """A random triangle soup around the origin. Face 0 is a large triangle behind the others (so that a 1 x 1 image hits something
    whatever else there is); every 50th face from the 25th repeats a vertex (skipped); two faces are listed twice (ties in t: the
    lower index wins, within a chunk and across chunks)."""
    rs = np.random.RandomState(2000 + nf)
    nv = max(3, min(300, nf)) + 3
    v = (rs.randn(nv, 3) * 0.6).astype(np.float32)
    v[:3] = [[-2.5, 1.0, -1.9], [2.6, 1.2, -1.7], [0.1, 0.9, 2.8]]
    f = rs.randint(3, nv, (nf, 3)).astype(np.int32)
    f[25::50, 1] = f[25::50, 0]
    f[0] = [0, 1, 2]
    if nf > 300:
        f[nf - 1] = f[2]
        f[260] = f[7]
    return v, f


@functools.lru_cache(maxsize=None)
def _soup_camera(hw):
    """A generic camera per image size: rotated, rolled, off-centre principal point, looking at the soup from y < 0 (mesh frame)."""
    H, W = hw
    rs = np.random.RandomState(H * 1000 + W)
    eye = np.array([rs.uniform(-0.6, 0.6), -2.4, rs.uniform(-0.5, 0.5)])
    RT = Q.look_at(M64 @ eye, M64 @ (rs.randn(3) * 0.05), roll_deg=rs.uniform(-40, 40))
    K = Q.intrinsic(H, W, f=1.3 * max(H, W, 8), cx=(W - 1) / 2 + 0.3, cy=(H - 1) / 2 - 0.2)
    return K, RT


FACE_COUNTS = (1, TILE - 1, TILE, TILE + 1, CH - 1, CH, CH + 1, 2 * CH + 1)
IMAGES = ((1, 1), (17, 15), (16, 16), (257, 1), (27, 19))        # H * W = 1, MB - 1, MB, MB + 1; 513: two blocks of k_mesh_cast


@pytest.mark.parametrize('hw', IMAGES)
@pytest.mark.parametrize('nf', FACE_COUNTS)
def test_random_soups_equal_restatement(nf, hw):
    v, f = _soup(nf)
    K, RT = _soup_camera(hw)
    hits = 0
    for frame in ('image', 'world'):
        got = _render(v, f, K, RT, hw, frame=frame)
        want = Q.render(v, f, Q.k_inv(K), Q.M_DEFAULT, RT, hw[0], hw[1], normal_frame=frame)
        _equals_restatement(got, want)
        hits = int(got['mask'].sum())
        assert (got['face'][got['mask'] == 0] == -1).all() and (got['depth'][got['mask'] == 0] == np.float32(1e11)).all()
    assert hits >= 0.5 * hw[0] * hw[1]
    if nf > 300 and hw == (17, 15):
        assert not np.isin(got['face'], [nf - 1, 260]).any() and want['nhits'].max() >= 3


# ------------------------------------------------------------------------------------------------------- invariance
@functools.lru_cache(maxsize=None)
def _sphere_mesh():
    v, f = R.marching_cubes(R.sphere_grid(24, (0.03, -0.02, 0.01), 0.5))
    assert (R.edge_use_counts(f) == 2).all() and len(f) > CH
    return v, f


def _orbit(n):
    return np.stack([Q.look_at(M64 @ np.array([2.2 * np.cos(0.7 * k), 2.2 * np.sin(0.7 * k), 0.4 * np.sin(0.3 * k)]), roll_deg=5.0 * k)
                     for k in range(n)])


def test_runs_repeat_and_views_equal_their_stand_alone_calls():
    v, f = _sphere_mesh()
    hw = (20, 23)
    K = Q.intrinsic(*hw, f=45.0)
    for B in (1, 2, 3, 65):                                        # 65: two pieces (64 + 1)
        RT = _orbit(B)
        a, b = _render(v, f, K, RT, hw), _render(v, f, K, RT, hw)
        _same_bytes(a, b)
        assert 100 < a['mask'][0].sum() < 400
        for i in sorted({0, B // 2, B - 1}):
            one = _render(v, f, K, RT[i], hw)
            _same_bytes({k: x[i] for k, x in a.items()}, one)
    _equals_restatement({k: x[64] for k, x in a.items()}, Q.render(v, f, Q.k_inv(K), Q.M_DEFAULT, RT[64], *hw))
    # a closed mesh: no hole inside the silhouette, and a view whose RT is not finite sees nothing
    bad = RT[:3].copy()
    bad[1, 2, 3] = np.nan
    c = _render(v, f, K, bad, hw)
    assert not c['mask'][1].any() and (c['face'][1] == -1).all() and (c['normal'][1] == 0).all()
    _same_bytes({k: x[[0, 2]] for k, x in c.items()}, {k: x[[0, 2]] for k, x in a.items()})


def test_skipped_faces_change_no_byte_and_winding_changes_no_depth():
    v, f = S.box()
    v2 = np.concatenate([v, [[0.25, 0.25, 0.25], [0.375, 0.375, 0.375], [1, 1, 1], [np.nan, 0, 0]]]).astype(np.float32)
    extra = np.array([[3, 3, 6], [8, 9, 10], [0, 1, 12], [0, -1, 2], [4, 11, 5]], np.int32)   # duplicate vertex, collinear, out of range, NaN
    hw = (33, 31)
    K = Q.intrinsic(*hw)
    RT = np.stack([Q.look_at(M64 @ np.array([1.2, -1.5, 0.9]), roll_deg=12), Q.look_at(M64 @ np.array([0.1, -0.2, 0.15]), M64 @ np.array([0.5, 0.4, 0.3]))])
    plain = _render(v, f, K, RT, hw)
    assert 100 < plain['mask'][0].sum() < 900 and plain['mask'][1].all()          # from outside; from inside: every ray hits
    _same_bytes(plain, _render(v2, np.concatenate([f, extra]), K, RT, hw))
    none = _render(v2, extra, K, RT, hw)
    assert not none['mask'].any() and (none['face'] == -1).all() and (none['depth'] == np.float32(1e11)).all()
    vi, fi = S.box(inward=True)
    inward = _render(vi, fi, K, RT, hw)
    _same_bytes(plain, inward, ('depth', 'zdepth', 'mask', 'normal'))
    for view in range(2):
        _equals_restatement({k: x[view] for k, x in inward.items()}, Q.render(vi, fi, Q.k_inv(K), Q.M_DEFAULT, RT[view], *hw))


# ------------------------------------------------------------------------------------------------------- the renderer
def _module(fixture_decoder):
    import torch
    from core.graph.deep_sdf_decoder import Decoder
    Ws, bs, latent = fixture_decoder
    dec = Decoder(256, [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(a) for l, (W, b) in enumerate(zip(Ws, bs)) for n, a in (('weight', W), ('bias', b))})
    return dec.cuda().eval(), torch.from_numpy(latent).cuda()


def test_renderer_method_equals_the_function(fixture_decoder):
    import torch
    from core.sdfrenderer import SDFRenderer
    from distr import mesh
    dec, _ = _module(fixture_decoder)
    hw = (21, 34)
    K = Q.intrinsic(*hw, f=40.0, cx=15.5, cy=11.0)
    Mx = np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0]], np.float64)              # not the default: the renderer's own matrix must travel
    ren = SDFRenderer(dec, K, img_hw=hw, transform_matrix=Mx)
    v, f = _sphere_mesh()
    RT = np.stack([Q.look_at(Mx @ np.array([1.9, 0.8, -0.7]), roll_deg=-20), Q.look_at(Mx @ np.array([-0.4, 2.1, 0.3]))])
    vt, ft, rt = _cuda(v), _cuda(f), _cuda(RT)
    for frame in ('image', 'world'):
        a = ren.render_mesh(vt, ft, rt[:, :, :3], rt[:, :, 3], normal_frame=frame, details=True)
        b = mesh.render_mesh(vt, ft, ren.get_intrinsic(), rt, ren.get_img_hw(), transform_matrix=Mx, normal_frame=frame, details=True)
        assert len(a) == 6 and all(torch.equal(x, y) and x.dtype == y.dtype for x, y in zip(a, b))
        one = ren.render_mesh(v, f, RT[1, :, :3], RT[1, :, 3], normal_frame=frame)              # numpy in, one view, no details
        assert len(one) == 3 and all(torch.equal(x, y[1]) for x, y in zip(one, b))
    assert 50 < int(a[2][0].sum()) < 600
    _equals_restatement({k: x[0].cpu().numpy() for k, x in zip(KEYS, a)}, Q.render(v, f, Q.k_inv(K), Mx, RT[0], *hw, normal_frame='world'))


TRACER_N = 64          # the smallest grid of (64, 128) at which the mask condition below holds on the CPU (oracle + restatement)


@functools.lru_cache(maxsize=None)
def _tracer_case(decoder):
    """The fixture decoder sphere-traced at 64 x 64 and its own marching-cubes mesh rendered from the same camera."""
    import torch
    from core.evaluation import create_sdf_grid
    from core.sdfrenderer import SDFRenderer_deepsdf
    from distr import fixture, mesh
    dec, lat = decoder
    H = W = 64
    ren = SDFRenderer_deepsdf(dec, fixture.make_intrinsic(H, W), img_hw=(H, W))
    ren.use_depth2normal = False
    Rm, T = fixture.make_camera(30, 20, 1.6, 10)
    Rt, Tt = _cuda(Rm), _cuda(T)
    with torch.no_grad():
        depth, normal, mask = ren.render(lat, Rt, Tt, no_grad=True)[:3]
        grid = create_sdf_grid(dec, lat, TRACER_N)
    v, f = mesh.marching_cubes(grid, 0.0, voxel_size=2.0 / (TRACER_N - 1))
    return ren, lat, Rt, Tt, v, f, depth, normal, mask


def _neighbour_has(mask, val):
    """Per pixel: is there a pixel of value `val` among its 8 neighbours."""
    m = np.pad(mask == val, 1)
    H, W = mask.shape
    acc = np.zeros(mask.shape, bool)
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                acc |= m[dy:dy + H, dx:dx + W]
    return acc


def test_against_the_sphere_tracer(fixture_decoder):
    """Mask: every pixel where the two masks differ has a pixel of the other value among its 8 neighbours in the sphere-traced mask
    (a silhouette pixel). Normals: over the pixels valid in both, the sum of the products is positive for each component -- a missing
    x flip, a missing R, a missing M or an inverted orientation each turn at least one of them."""
    import torch
    ren, lat, Rt, Tt, v, f, depth, normal, mask = _tracer_case(_cached_module(fixture_decoder))
    assert (R.edge_use_counts(f.cpu().numpy()) == 2).all()
    d, n, m = ren.render_mesh(v, f, Rt, Tt)
    assert d.shape == depth.shape and n.shape == normal.shape and m.shape == mask.shape
    assert d.dtype == depth.dtype and n.dtype == normal.dtype and m.dtype == mask.dtype
    ms, mm = mask.cpu().numpy().astype(bool), m.cpu().numpy().astype(bool)
    assert 500 < ms.sum() < 64 * 64 - 500
    diff = ms != mm
    other = np.where(ms, _neighbour_has(ms, False), _neighbour_has(ms, True))
    print('masks differ at %d of %d valid pixels' % (diff.sum(), ms.sum()))
    assert not (diff & ~other).any(), int((diff & ~other).sum())
    both = ms & mm
    a, b = n.cpu().numpy()[both].astype(np.float64), normal.cpu().numpy()[both].astype(np.float64)
    sums = (a * b).sum(0)
    dd = np.abs(d.cpu().numpy() - depth.cpu().numpy())[both]
    ang = np.degrees(np.arccos(np.clip((a * b).sum(1) / np.maximum(np.linalg.norm(b, axis=1), 1e-30), -1, 1)))
    print('N = %d, %d faces: |depth difference| max %.3g median %.3g; mean angle between normals %.3g deg; component sums %s'
          % (TRACER_N, len(f), dd.max(), np.median(dd), ang.mean(), sums))
    assert (sums > 0).all(), sums
    assert (d[~m.bool()] == 1e11).all() and bool(torch.isfinite(n).all())


_modules = {}


def _cached_module(fixture_decoder):
    if 'm' not in _modules:
        _modules['m'] = _module(fixture_decoder)
    return _modules['m']


def test_maps_into_get_samples(fixture_decoder):
    """The mesh-rendered depth and 'world' normals are what get_samples takes: with the decoder's own code the residuals
    f(p + eta n) - eta and f(p - eta n) + eta stay below eta on average (a flipped normal gives about 2 eta, a depth in the wrong
    convention the clamp distance)."""
    import torch
    ren, lat, Rt, Tt, v, f, _, _, _ = _tracer_case(_cached_module(fixture_decoder))
    eta = 0.01
    depth, normal, mask = ren.render_mesh(v, f, Rt, Tt, normal_frame='world')
    RT = torch.cat([Rt, Tt[:, None]], 1)
    with torch.no_grad():
        pos, neg = ren.get_samples(lat, RT, depth, normal, use_rand=False, eta=eta)
    assert pos.shape == neg.shape == (int(mask.sum()),)
    print('mean |samples_pos| %.3g, mean |samples_neg| %.3g (eta %.3g)' % (float(pos.abs().mean()), float(neg.abs().mean()), eta))
    assert float(pos.abs().mean()) < eta and float(neg.abs().mean()) < eta


def test_refusals():
    import torch
    from distr import binding, mesh
    v, f = S.box()
    vt, ft = _cuda(v), _cuda(f)
    K, RT = Q.intrinsic(8, 8), _cuda(Q.look_at([0.0, -2.0, 0.0]))
    with pytest.raises(ValueError, match='no triangles'):
        mesh.render_mesh(vt, ft[:0], K, RT, (8, 8))
    with pytest.raises(ValueError, match=r'RT has shape \(4, 3\)'):
        mesh.render_mesh(vt, ft, K, RT.t().contiguous(), (8, 8))
    with pytest.raises(ValueError, match=r'RT has shape \(2, 3, 3\)'):
        mesh.render_mesh(vt, ft, K, RT[None, :, :3].repeat(2, 1, 1), (8, 8))
    with pytest.raises(ValueError, match="normal_frame 'camera'"):
        mesh.render_mesh(vt, ft, K, RT, (8, 8), normal_frame='camera')
    # the C ABI: no faces, a wrong struct_size, a short workspace, too many views
    ctx = mesh._context(torch.device('cuda', 0))
    cfg = binding.make_mesh_render_cfg((8, 8), K, Q.M_DEFAULT, 'image')
    out = torch.empty(64, device='cuda')
    ws = torch.empty(ctx.L.distr_mesh_render_workspace_bytes(8, 8, 1), dtype=torch.uint8, device='cuda')
    import ctypes as C

    def call(cfg=cfg, nf=len(f), nviews=1, ws_bytes=ws.numel()):
        return ctx.L.distr_mesh_render(ctx.h, C.byref(cfg), binding.ptr(vt), len(v), binding.ptr(ft), nf, nviews, binding.ptr(RT), binding.ptr(out),
                                       None, None, None, None, None, binding.ptr(ws), ws_bytes, None)
    assert call() == 0
    torch.cuda.synchronize()
    assert 10 < int((out < 1e5).sum()) < 64
    assert call(nf=0) == -1 and 'triangles' in ctx.L.distr_last_error(ctx.h).decode()
    assert call(nviews=65) == -1 and call(nviews=0) == -1
    assert call(ws_bytes=ws.numel() - 1) != 0 and 'workspace' in ctx.L.distr_last_error(ctx.h).decode()
    short = binding.make_mesh_render_cfg((8, 8), K, Q.M_DEFAULT, 'image')
    short.struct_size -= 4
    assert call(cfg=short) == -1 and 'struct_size' in ctx.L.distr_last_error(ctx.h).decode()
    frame = binding.make_mesh_render_cfg((8, 8), K, Q.M_DEFAULT, 'image')
    frame.normal_frame = 2
    assert call(cfg=frame) == -1
