"""TEST INFRASTRUCTURE -- golden G31: SDFRenderer_deepsdf.get_samples / get_freespace_samples evaluated by the REFERENCE itself on CPU
(build container only: imports the reference through the unchanged oracle/ref_harness.py; no reference source is copied, the output
is arrays and short key strings):

    python tests/gen_golden_depth_samples.py        # writes tests/golden/g31_depth_samples.npz

Scenes: fixtures F1 and F2, 40 x 48 images, a rotated camera; the observation (depth, normal) is the reference's own `render` of a
nearby but different shape code, so the residuals are not zero. Cases per fixture (keys `<fixture>_<case>_*`):
    s_rand   get_samples, use_rand=True,  clamp_dist 0.1          f_n1   get_freespace_samples, number 1, clamp_dist 0.1
    s_fix    get_samples, use_rand=False, clamp_dist 0.1          f_n3   get_freespace_samples, number 3, clamp_dist 0.5
    s_clamp  get_samples, use_rand=True,  clamp_dist 0.004 (some samples clamp)
The random draws are pinned: torch.rand_like is substituted, in this process, by a function that hands out recorded arrays (the
reference's files are not edited). Recorded per case: all inputs and draws, the outputs, recorded weights w, the gradients of
(w . out).sum() w.r.t. the latent code and RT, and -- for the knife-edge check -- the gradient w.r.t. the points the decoder saw
(decode_sdf of the reference module is wrapped to keep them).

Noise floors (`*_floor_*`): the same case three more times with the decoder weights AND RT and depth perturbed by 1e-7 relative (this
build computes the points in another f32 order than torch, so the decoder sees slightly different inputs, not only other weights); the
maximum residual over the draws. Knife-edge check, asserted here: under each noise draw at most one sample's point gradient moves by
more than 1e-3 relative (a hidden unit whose pre-activation is ~1e-8 sits on either side of its ReLU: the allowance G11 carries)."""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, '..', 'dist-renderer_amd'))
sys.path.insert(0, os.path.join(_HERE, '..', 'oracle'))
from distr import fixture  # noqa: E402
import ref_harness as rh  # noqa: E402

OUT = os.path.join(_HERE, 'golden', 'g31_depth_samples.npz')
H, W = 40, 48
ETA = 0.01
CASES = (('s_rand', 'samples', dict(use_rand=True, clamp_dist=0.1)), ('s_fix', 'samples', dict(use_rand=False, clamp_dist=0.1)),
         ('s_clamp', 'samples', dict(use_rand=True, clamp_dist=0.004)), ('f_n1', 'free', dict(number=1, clamp_dist=0.1)),
         ('f_n3', 'free', dict(number=3, clamp_dist=0.5)))
NOISE_DRAWS = 3
SEEDS = {'f1': 31, 'f2': 38}      # scene seeds (f2: 32..37 put two or more samples on a knife edge for the reference itself, see below)


class Draws(object):
    """Stands in for torch.rand_like: hands out the queued arrays, one per call."""

    def __init__(self):
        self.queue = []

    def __call__(self, t, *a, **k):
        r = self.queue.pop(0)
        assert r.shape == tuple(t.shape), (r.shape, tuple(t.shape))
        return torch.from_numpy(r.copy())


class PointTap(object):
    """Wraps the reference module's decode_sdf: keeps the points of every call on the tape (their gradient = the per-sample one)."""

    def __init__(self, fn):
        self.fn, self.points = fn, []

    def __call__(self, decoder, latent, points, **k):
        points.retain_grad()
        self.points.append(points)
        return self.fn(decoder, latent, points, **k)


def run_case(mod, rend, kind, kw, latent, RT, depth, normal, draws_np, w_np, draws):
    """One reference call + backward of (w . out).sum() -> dict of arrays."""
    lat = torch.from_numpy(latent.copy()).requires_grad_(True)
    rt = torch.from_numpy(RT.copy()).requires_grad_(True)
    d = torch.from_numpy(depth.copy())
    tap = PointTap(mod.decode_sdf.fn if isinstance(mod.decode_sdf, PointTap) else mod.decode_sdf)
    mod.decode_sdf = tap
    draws.queue = [r for r in draws_np]
    if kind == 'samples':
        pos, neg = rend.get_samples(lat, rt, d, torch.from_numpy(normal.copy()), eta=ETA, **kw)
        out = torch.cat([pos, neg])
    else:
        out = rend.get_freespace_samples(lat, rt, d, **kw)
    assert not draws.queue or (kind == 'samples' and not kw['use_rand'])
    (out * torch.from_numpy(w_np)).sum().backward()
    g_points = torch.cat([p.grad if p.grad is not None else torch.zeros_like(p) for p in tap.points]).numpy()
    return dict(out=out.detach().numpy(), g_latent=lat.grad.numpy().copy(), g_RT=rt.grad.numpy().copy(), g_points=g_points,
                points=torch.cat([p.detach() for p in tap.points]).numpy())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    rh.reference_modules()
    import core.sdfrenderer.renderer_deepsdf as mod
    assert os.path.abspath(mod.__file__).startswith(rh.REFERENCE_ROOT)
    draws = Draws()
    torch.rand_like = draws
    K = fixture.make_intrinsic(H, W)
    R, T = fixture.make_camera(35, 25, 1.6, 15)
    RT = np.concatenate([R, T.reshape(3, 1)], 1).astype(np.float32)
    out = dict(K=K, H=H, W=W, eta=np.float32(ETA), noise_draws=NOISE_DRAWS, case_names=np.array([c[0] for c in CASES]),
               fixtures=np.array(['f1', 'f2']))
    for fx, (Ws, bs, latent) in (('f1', fixture.make_decoder_weights()), ('f2', fixture.load_fixture_f2())):
        rs = np.random.RandomState(SEEDS[fx])
        dec = rh.build_reference_decoder(Ws, bs)
        rend = mod.SDFRenderer_deepsdf(dec, K, img_hw=(H, W), use_gpu=False)
        # the observation: the reference's own render of a nearby code
        lat_obs = (latent + 0.02 * np.abs(latent).max() * rs.standard_normal(latent.shape)).astype(np.float32)
        dimg, nimg = rend.render(torch.from_numpy(lat_obs), torch.from_numpy(RT[:, :3].copy()), torch.from_numpy(RT[:, 3].copy()), no_grad=True)[:2]
        depth, normal = dimg.detach().numpy().astype(np.float32).reshape(H, W), nimg.detach().numpy().astype(np.float32).reshape(H, W, 3)
        valid = (depth > 0) & (depth < 1e5)
        N = int(valid.sum())
        assert 100 < N < H * W, N
        out.update({fx + '_latent': latent, fx + '_RT': RT, fx + '_depth': depth, fx + '_normal': normal, fx + '_N': N,
                    fx + '_weights_sha256': fixture.weights_sha256(Ws, bs)})
        # perturbed copies for the noise floors: decoder weights AND RT and depth, 1e-7 relative
        noisy = []
        for sd in range(NOISE_DRAWS):
            rn = np.random.RandomState(310 + sd)
            Wn = [(Wl * (1 + 1e-7 * rn.standard_normal(Wl.shape))).astype(np.float32) for Wl in Ws]
            noisy.append((mod.SDFRenderer_deepsdf(rh.build_reference_decoder(Wn, bs), K, img_hw=(H, W), use_gpu=False),
                          (RT * (1 + 1e-7 * rn.standard_normal(RT.shape))).astype(np.float32),
                          np.where(valid, depth * (1 + 1e-7 * rn.standard_normal(depth.shape)), depth).astype(np.float32)))
        for name, kind, kw in CASES:
            m = 2 if kind == 'samples' else kw['number']
            if kind == 'samples':
                dr = [rs.random_sample(N).astype(np.float32)] if kw['use_rand'] else []
                eta_map = dr[0] * np.float32(ETA) if dr else np.full(N, ETA, np.float32)
                out['%s_%s_eta_map' % (fx, name)] = eta_map.astype(np.float32)
            else:
                dr = [rs.random_sample(N).astype(np.float32) for _ in range(m)]
                out['%s_%s_ratio' % (fx, name)] = np.stack(dr)
            w = rs.uniform(0.5, 1.5, m * N).astype(np.float32) * rs.choice([-1.0, 1.0], m * N).astype(np.float32)
            a = run_case(mod, rend, kind, kw, latent, RT, depth, normal, dr, w, draws)
            key = '%s_%s_' % (fx, name)
            out.update({key + 'w': w, key + 'out': a['out'], key + 'g_latent': a['g_latent'], key + 'g_RT': a['g_RT'],
                        key + 'g_points': a['g_points'], key + 'clamp_dist': np.float32(kw['clamp_dist'])})
            if kind == 'samples':
                inner = np.abs(a['out'] + np.concatenate([eta_map, -eta_map])) < kw['clamp_dist']
                print(key, 'N', N, 'unclamped', int(inner.sum()), 'of', 2 * N, flush=True)
                if name == 's_clamp':
                    assert 0 < inner.sum() < 2 * N, 'the small clamp_dist must clamp some samples, not all'
            fl, moved = dict(out=0.0, g_latent_rel=0.0, g_R_rel=0.0, g_T_rel=0.0), []
            for rend_n, RT_n, depth_n in noisy:
                b = run_case(mod, rend_n, kind, kw, latent, RT_n, depth_n, normal, dr, w, draws)
                fl['out'] = max(fl['out'], float(np.abs(a['out'] - b['out']).max()))
                fl['g_latent_rel'] = max(fl['g_latent_rel'], float(np.abs(a['g_latent'] - b['g_latent']).max() / np.abs(a['g_latent']).max()))
                for k, sl in (('g_R_rel', np.s_[:, :3]), ('g_T_rel', np.s_[:, 3])):
                    fl[k] = max(fl[k], float(np.abs(a['g_RT'][sl] - b['g_RT'][sl]).max() / np.abs(a['g_RT'][sl]).max()))
                moved.append(int((np.abs(a['g_points'] - b['g_points']).max(1) > 1e-3 * np.abs(a['g_points']).max()).sum()))
            print(key, 'samples whose point gradient moved by > 1e-3 relative, per noise draw:', moved, flush=True)
            assert max(moved) <= 1, '%s: %s samples on a ReLU knife edge under the generator\'s own noise: pick another seed' % (key, moved)
            out.update({key + 'floor_' + k: np.float64(v) for k, v in fl.items()})
            print(key, 'floors', fl, flush=True)
    np.savez_compressed(OUT, **out)
    print('g31 done:', len(out), 'arrays,', os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
