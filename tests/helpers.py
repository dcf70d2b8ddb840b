"""Shared helpers of the GPU parity tests (HIP kernels through the C ABI vs the CPU oracle)."""
import numpy as np


def loss_weights(H, W, seed):
    rs = np.random.RandomState(seed)
    return rs.rand(H, W).astype(np.float32), rs.rand(H, W).astype(np.float32), rs.rand(H, W, 3).astype(np.float32)


def oracle_render(O, orc, H, W, K, R, T, latent, seed=5, **kw):
    cfg = orc.make_cfg(H, W, K, **kw)
    out = O.render(cfg, latent, R, T)
    wd, wq, wn = loss_weights(H, W, seed)
    m = out['mask'].reshape(H, W).astype(np.float32)
    gl, gR, gT, ns = out['state'].backward(g_min_sdf=wq.reshape(-1), g_depth=(wd * m).reshape(-1), g_normal=wn.reshape(-1))
    out.update(g_latent=gl, g_R=gR, g_T=gT, num_samples=ns, num_evals=out['state'].num_evals)
    mb = m.astype(bool)
    out['loss'] = float((out['depth'].reshape(H, W).astype(np.float64) * wd)[mb].sum() + (out['min_sdf'].reshape(H, W).astype(np.float64) * wq).sum() +
                        (out['normal'].reshape(H, W, 3).astype(np.float64) * wn).sum())
    return out


def hip_render(engine, H, W, K, R, T, latent, seed=5, **kw):
    """Same computation through libdistr (torch only owns the buffers / runs the tiny loss)."""
    import torch
    from distr import binding, functions
    dev = engine.device
    cfg = binding.make_cfg((H, W), K, **kw)
    lat = torch.from_numpy(np.asarray(latent, np.float32)).to(dev).requires_grad_(True)
    Rt = torch.from_numpy(np.asarray(R, np.float32)).to(dev).requires_grad_(True)
    Tt = torch.from_numpy(np.asarray(T, np.float32)).to(dev).requires_grad_(True)
    zdepth, mask, min_sdf, depth, normal = functions.render_call(engine, cfg, lat, Rt, Tt)
    wd, wq, wn = (torch.from_numpy(a).to(dev) for a in loss_weights(H, W, seed))
    mb = mask.reshape(H, W).bool()
    L = (depth * wd)[mb].sum() + (min_sdf.reshape(H, W) * wq).sum() + (normal * wn).sum()
    L.backward()
    torch.cuda.synchronize()
    return dict(zdepth=zdepth.detach().cpu().numpy(), mask=mask.cpu().numpy(), min_sdf=min_sdf.detach().cpu().numpy(),
                depth=depth.detach().cpu().numpy(), normal=normal.detach().cpu().numpy(),
                g_latent=lat.grad.cpu().numpy(), g_R=Rt.grad.cpu().numpy(), g_T=Tt.grad.cpu().numpy(), cfg=cfg, loss=float(L.detach()))


def compare(a, b, H, W, tol_depth=1e-4, tol_grad=1e-3, normal_p99=1e-4, max_flip_frac=0.001):
    """a: HIP, b: oracle/golden dicts. Returns a dict of residuals after asserting the bars."""
    ma, mb = a['mask'].reshape(H, W).astype(bool), b['mask'].reshape(H, W).astype(bool)
    flips = int((ma != mb).sum())
    both = ma & mb
    res = dict(flips=flips,
               depth=float(np.abs(a['depth'] - b['depth'])[both].max()) if both.any() else 0.0,
               zdepth=float(np.abs(a['zdepth'].reshape(H, W) - b['zdepth'].reshape(H, W))[both].max()) if both.any() else 0.0,
               min_sdf=float(np.abs(a['min_sdf'].reshape(-1) - b['min_sdf'].reshape(-1)).max()),
               normal_p99=float(np.percentile(np.abs(a['normal'] - b['normal'])[both], 99)) if both.any() else 0.0,
               normal_max=float(np.abs(a['normal'] - b['normal'])[both].max()) if both.any() else 0.0)
    for k in ('g_latent', 'g_R', 'g_T'):
        res[k] = float(np.abs(a[k].reshape(-1) - b[k].reshape(-1)).max() / max(np.abs(b[k]).max(), 1e-30))
    assert flips <= max(1, int(max_flip_frac * H * W)), res
    assert res['depth'] <= tol_depth and res['zdepth'] <= tol_depth and res['min_sdf'] <= tol_depth, res
    assert res['normal_p99'] <= normal_p99, res
    assert max(res['g_latent'], res['g_R'], res['g_T']) <= tol_grad, res
    return res


def compare_big_golden(a, g, label, grad_floor_mult=2.0):
    """a: a render dict (HIP or oracle: mask / depth / zdepth / min_sdf / normal / g_*), g: one of the reference goldens generated at
    the sizes the metric is quoted on (oracle/gen_golden_big.py: G15 = C3 512^2/50, G16 = one C5 image 1024^2/100). The golden holds the
    full mask bit-packed, every `sub`-th pixel of every image exactly, four 32x32 crops, per-row depth sums, the loss, the gradients
    and the reference's own noise floor (same render with 1e-7 relative weight noise). Bars: north_star's 1e-4 on depth / Zdepth /
    min-sdf (min-sdf: at least 2x its recorded floor, which sits at 0.94e-4), normals at the p99 bar of the G3 tests, gradients and
    loss within `grad_floor_mult` x the floor. Returns the residuals (printed by the caller next to the floor)."""
    H, W, sub = int(g['H']), int(g['W']), int(g['sub'])
    gm = np.unpackbits(g['mask_bits'])[:H * W].reshape(H, W).astype(bool)
    am = a['mask'].reshape(H, W).astype(bool)
    flips = int((am != gm).sum())
    res = {'flips': flips, 'valid': int(am.sum()), 'valid_ref': int(g['valid_count'])}
    assert int(gm.sum()) == int(g['valid_count'])
    assert flips <= max(2, int(1e-4 * int(g['valid_count']))), (label, res)
    depth, z, q, nrm = a['depth'].reshape(H, W), a['zdepth'].reshape(H, W), a['min_sdf'].reshape(H, W), a['normal'].reshape(H, W, 3)
    fx = float(g['K'][0, 0])
    bar_q = max(1e-4, 2.0 * float(g['floor_min_sdf']))
    bar_d = max(1e-4, 2.0 * float(g['floor_depth']))
    bar_n = max(1e-4, 1e-5 * fx, 2.0 * float(g['floor_normal_p99']))      # finite differences amplify depth noise by fx / 2

    def region(ad, az, aq, an, am_, gd, gz, gq, gn, gmask, name):
        both = am_ & gmask.astype(bool)
        none = ~(am_ | gmask.astype(bool))
        r = {}
        if both.any():
            r['depth'] = float(np.abs(ad - gd)[both].max())
            r['zdepth'] = float(np.abs(az - gz)[both].max())
            r['depth_px_over_1e-4'] = int((np.abs(ad - gd)[both] > 1e-4).sum())
            dn = np.abs(an - gn)[both]
            r['normal_p99'] = float(np.percentile(dn, 99))
            r['normal_max'] = float(dn.max())
            # 1e-4, except where the reference's own depth moves by more under 1e-7 weight noise (a stop-step event on an isolated
            # pixel: G16's floor is 1.46e-4): then 2 x that floor, and at most 1 pixel in 10 000 above 1e-4
            assert r['depth'] <= bar_d and r['zdepth'] <= bar_d, (label, name, r, bar_d)
            assert r['depth_px_over_1e-4'] <= max(1, int(1e-4 * int(both.sum()))), (label, name, r)
            assert r['normal_p99'] <= bar_n, (label, name, r, bar_n)
        r['min_sdf'] = float(np.abs(aq - gq).max())
        assert r['min_sdf'] <= bar_q, (label, name, r, bar_q)
        assert np.array_equal(ad[none], gd[none])          # background convention of depth2normal (0) / render (1e11): exact
        return r
    res['sub'] = region(depth[::sub, ::sub], z[::sub, ::sub], q[::sub, ::sub], nrm[::sub, ::sub], am[::sub, ::sub],
                        g['sub_depth'], g['sub_zdepth'], g['sub_q'], g['sub_normal'], gm[::sub, ::sub], 'sub-grid')
    for i in range(4):
        y0, x0 = (int(v) for v in g['crop%d_yx' % i])
        sl = (slice(y0, y0 + 32), slice(x0, x0 + 32))
        assert np.array_equal(g['crop%d_mask' % i].astype(bool), gm[sl])
        res['crop%d' % i] = region(depth[sl], z[sl], q[sl], nrm[sl], am[sl], g['crop%d_depth' % i], g['crop%d_zdepth' % i],
                                   g['crop%d_min_abs_query' % i], g['crop%d_normal' % i], g['crop%d_mask' % i], 'crop %d' % i)
    # whole-image sums: rows whose masks agree compare their depth sums (f64) at 1e-4 per valid pixel
    same_rows = (am == gm).all(1)
    rs = np.where(am, depth, 0).astype(np.float64).sum(1)
    cnt = np.maximum(am.sum(1), 1)
    rows = (np.abs(rs - g['row_sum_depth']) / cnt)[same_rows]
    res['row_mean_depth'] = float(rows.max())
    res['rows_over_1e-4'] = int((rows > 1e-4).sum())
    # a row's mean moves by more than 1e-4 only through an isolated stop-step pixel in a row with few valid pixels (the reference's own
    # floor_depth says how far such a pixel can move): bounded by that floor, and rare
    assert res['row_mean_depth'] <= bar_d and res['rows_over_1e-4'] <= max(1, H // 200), (label, res)
    res['mean_q'] = float(abs(q.astype(np.float64).sum() - float(g['sum_q'])) / (H * W))
    assert res['mean_q'] <= 1e-5, (label, res)
    if 'loss' in a:
        res['loss_rel'] = float(abs(a['loss'] - float(g['loss'])) / abs(float(g['loss'])))
        assert res['loss_rel'] <= max(1e-5, grad_floor_mult * float(g['floor_loss_rel'])), (label, res)
    for k in ('g_latent', 'g_R', 'g_T'):
        if k not in g:                 # a forward-only golden (G16: the reference's autograd tape at 1024^2 does not fit the build container)
            continue
        rel = float(np.abs(a[k].reshape(-1) - g[k].reshape(-1)).max() / np.abs(g[k]).max())
        fl = float(g['floor_%s_rel' % k])
        res[k] = rel
        res[k + '_floor'] = fl
        assert rel <= grad_floor_mult * fl, (label, k, rel, fl)
    return res



# ---- the early break of the recursive march (renderer.py:562-567) at its edges: one random draw of the sweep and the class of its march
EARLY_BREAK_MENU = ([2, 1], [3, 1], [4, 2, 1], [4, 2, 1], [6, 2, 1], [8, 4, 2, 1])
EARLY_BREAK_CLASSES = ('below', 'last', 'none')
MAX_BS = 8                     # include/distr.h: largest buffer_size


def early_break_class(state, fine_steps):
    """'below': no ray live after step L - 1 < fine_steps - 1 with L < buffer_size (the lists are padded); 'last': the same on the last step
    of a fine level shorter than buffer_size (L = fine_steps); 'none': no padding (the march ran out of steps with a live ray, or broke at
    L >= buffer_size). From the oracle's state (oracle/oracle.py: fine_rows / padded)."""
    if not state.padded:
        return 'none'
    return 'last' if state.fine_rows == fine_steps else 'below'


def early_break_draw(seed, O, orc, latent):
    """Seeded draw of the early-break sweep: a pyramid (menu above) whose fine level has 1 .. buffer_size + 2 steps, buffer_size 2..8, a camera
    inside the sphere looking at the surface, exact sphere tracing (ratio 1) mostly. seed % 3 aims at one class: 0 'last' -- the scene is
    probed on the oracle (forward only, 12 fine steps, buffer_size 1), the fine level cut to the step L its march broke on and buffer_size
    drawn above L (the coarse levels stay and the march does not depend on buffer_size: the same march, ending on its last step);
    1 'below' (fine level >= buffer_size); 2 'none' (longer steps: the march outlasts the buffer or runs out).
    Returns (H, W, K, R, T, kw, fine_steps); the class is read from the oracle's render (early_break_class)."""
    from distr import fixture
    aim = seed % 3
    rs = np.random.RandomState(31000 + seed)
    H, W = int(rs.randint(24, 64)), int(rs.randint(24, 64))
    bs = int(rs.randint(2, 9))
    sl = list(EARLY_BREAK_MENU[rs.randint(len(EARLY_BREAK_MENU))])
    msl = [int(rs.randint(1, 4)) for _ in sl[:-1]]
    fine = int(rs.randint(bs, bs + 3)) if aim < 2 else int(rs.randint(1, bs + 3))
    while sum(msl) + fine < bs:         # (check_cfg: coarse rows + fine steps >= buffer_size)
        msl[int(rs.randint(len(msl)))] += 1
    kw = dict(march_step=sum(msl) + fine, buffer_size=bs, ratio=1.0 if aim < 2 else float(rs.choice([1.0, 1.5, 2.0])), marcher='pyramid_recursive',
              use_depth2normal=bool(rs.randint(2)), scale_list=sl, march_step_list=msl + [-1], threshold=float(10 ** rs.uniform(-3.2, -2.5)),
              radius=float(rs.uniform(1.0, 1.3)), clamp_dist=float(rs.uniform(0.1, 0.3)))
    cam = (float(rs.uniform(-180, 180)), float(rs.uniform(-60, 60)), float(rs.uniform(0.4, 0.6) if aim < 2 else rs.uniform(0.5, 0.8)), float(rs.uniform(-30, 30)))
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(*cam)
    if aim == 0:
        probe = dict(kw, march_step=sum(msl) + 12, buffer_size=1)
        st = O.render(orc.make_cfg(H, W, K, **probe), latent, R, T)['state']
        L = st.fine_rows
        if not st.live_after_last_step and 1 <= L < 12 and L + 1 <= min(MAX_BS, sum(msl) + L):
            fine = L
            kw.update(march_step=sum(msl) + L, buffer_size=int(rs.randint(L + 1, min(MAX_BS, sum(msl) + L) + 1)))
    return H, W, K, R, T, kw, fine


DEEPSDF_SPECS = {       # the layout of facebookresearch/DeepSDF's examples/*/specs.json (what load_decoder reads, decoder_utils.py:7-27)
    'Description': ['synthetic experiment directory written by tests/helpers.py: fixture F1 in DeepSDF checkpoint format'],
    'NetworkArch': 'deep_sdf_decoder', 'CodeLength': 256,
    'NetworkSpecs': {'dims': [512] * 8, 'dropout': list(range(8)), 'dropout_prob': 0.2, 'norm_layers': list(range(8)), 'latent_in': [4],
                     'xyz_in_all': False, 'use_tanh': False, 'latent_dropout': False, 'weight_norm': True},
}


def write_deepsdf_experiment(root, state_dict, checkpoint='2000', module_prefix=True, epoch=2000):
    """A DeepSDF experiment directory as the reference's drivers expect it (run_single_shape.py:26-33, decoder_utils.py:7-51):
    <root>/specs.json + <root>/ModelParameters/<checkpoint>.pth = {'epoch', 'model_state_dict'}; shape decoders are saved from a
    DataParallel module ('module.' prefix), colour decoders without it (decoder_utils.py:35-42). `state_dict`: name -> numpy array."""
    import json
    import os
    import torch
    os.makedirs(os.path.join(root, 'ModelParameters'), exist_ok=True)
    with open(os.path.join(root, 'specs.json'), 'w') as f:
        json.dump(DEEPSDF_SPECS, f)
    sd = {(('module.' + k) if module_prefix else k): torch.from_numpy(np.ascontiguousarray(v)) for k, v in state_dict.items()}
    torch.save({'epoch': epoch, 'model_state_dict': sd}, os.path.join(root, 'ModelParameters', checkpoint + '.pth'))
    return root


# ---- the few FULL-SIZE oracle renders of the GPU suite (one 512 x 512 oracle render = ~20 s of all host cores, the 1024 x 1024 / 100-step one
# ~85 s: a third of the suite's wall time in round 5). They are independent of the GPU, so a background thread renders them from the
# start of the session (tests/conftest.py: the tests that need them run LAST) while the other tests use the GPU; ctypes releases the GIL
# inside the oracle. key -> (image side, camera of the C4 circle, march steps); all: pyramid_recursive, buffer 3, depth2normal, dense loss.
BIG_ORACLE = {'c5_image0': (1024, 0, 100), 'c3': (512, 0, 50), 'c4_view1': (512, 1, 50), 'c4_view3': (512, 3, 50), 'c4_view5': (512, 5, 50),
              'c4_view7': (512, 7, 50), 'c4_view2': (512, 2, 50), 'c4_view4': (512, 4, 50), 'c4_view6': (512, 6, 50)}
_big = {'thread': None, 'results': {}, 'events': {}, 'errors': {}}


def bench_camera(view):
    """The cameras of bench.py (8 on a circle around the object)."""
    from distr import fixture
    return fixture.make_camera(45.0 * view, 25.0 if view else 0.0, 1.6, 0.0) if view else fixture.make_camera(0, 0, 1.6, 0)


def _big_oracle_render(key, O, orc, latent):
    from distr import fixture
    size, view, steps = BIG_ORACLE[key]
    K = fixture.make_intrinsic(size, size)
    R, T = bench_camera(view)
    return oracle_render(O, orc, size, size, K, R, T, latent, march_step=steps, buffer_size=3, marcher='pyramid_recursive', use_depth2normal=True)


def start_big_oracle(O, orc, latent, keys):
    """Background thread: the renders of `keys` one after the other (each already uses every core)."""
    import threading
    if _big['thread'] is not None:
        return
    for k in keys:
        _big['events'][k] = threading.Event()

    def work():
        # half the cores for this thread's OpenMP regions (omp_set_num_threads is per calling thread): the foreground tests run oracle
        # renders and multi-process loops of their own -- two full-width teams thrash (round 6, first try: the suite got no faster)
        try:
            orc.lib().orc_set_num_threads(max(8, orc.lib().orc_num_threads() // 2))
        except Exception:
            pass
        for k in keys:
            try:
                _big['results'][k] = _big_oracle_render(k, O, orc, latent)
            except BaseException as e:          # (re-raised in the test that asks for the result)
                _big['errors'][k] = e
            _big['events'][k].set()
    _big['thread'] = threading.Thread(target=work, name='big-oracle-prefetch', daemon=True)
    _big['thread'].start()


def big_oracle(key, O, orc, latent):
    """The oracle's fwd + bwd result of BIG_ORACLE[key]: from the prefetch thread if it is (being) rendered there, else rendered now."""
    ev = _big['events'].get(key)
    if ev is None:
        return _big_oracle_render(key, O, orc, latent)
    ev.wait()
    if key in _big['errors']:
        raise _big['errors'][key]
    return _big['results'].pop(key)
