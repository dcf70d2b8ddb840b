"""TEST INFRASTRUCTURE -- golden G30: the early break of the recursive march on the LAST step of a pyramid's fine level that is shorter than
buffer_size, rendered fwd + bwd by the REFERENCE itself on CPU (build container only; shims in oracle/ref_harness.py; no reference source
copied):

    python oracle/gen_golden_short_fine_break.py        # writes tests/golden/g30_short_fine_break.npz

ray_marching_recursive (core/sdfrenderer/renderer.py:562-567) pads its lists to buffer_size rows by repeating the last step's rows whenever no
ray is unfinished after a step -- the last step of the loop included. A pyramid's fine level can be shorter than buffer_size (its coarse rows
fill the buffer), so the break can come on that level's last step: the selection then holds copies of a ray's last row, each with the row's
gradient, exactly as for a break before it (G29). Scene of G29 (camera inside the sphere next to the surface, exact sphere tracing).
Cases: the default pyramid with march_step 7 and buffer_size 7 (fine level of 1 step; every ray finishes on it), a four-level
march_step_list pyramid whose fine level of 2 steps breaks on its last step (threshold 5e-4, buffer_size 8, autograd normals), and the control:
the same pyramid cut to 1 fine step (buffer_size 7), after which 121 rays are still unfinished -- no padding. Same layout and floors as G29
(gen_golden_early_break.py).
"""
import os
import sys

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(_HERE, '..', 'dist-renderer_amd'))
sys.path.insert(0, _HERE)
from distr import fixture  # noqa: E402
import ref_harness as rh  # noqa: E402
import gen_golden_options as go  # noqa: E402

OUT = os.path.join(_HERE, '..', 'tests', 'golden')
H, W = 55, 79
BASE = dict(ray_marching_ratio=1.0, radius=1.2)
PYR4 = dict(scale_list=[8, 4, 2, 1], march_step_list=[2, 2, 2, -1], threshold=5e-4)
CASES = {
    'pyramid_ms7_bs7_d2n': (dict(march_step=7, buffer_size=7, threshold=1.5e-3, use_depth2normal=True), dict(ray_marching_type='pyramid_recursive', clamp_dist=0.2)),
    'four_level_fine2_bs8': (dict(march_step=8, buffer_size=8, **PYR4), dict(ray_marching_type='pyramid_recursive', clamp_dist=0.2)),
    'four_level_fine1_bs7': (dict(march_step=7, buffer_size=7, **PYR4), dict(ray_marching_type='pyramid_recursive', clamp_dist=0.2)),
}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    K = np.array(fixture.make_intrinsic(H, W), dtype=np.float64)
    R, T = fixture.make_camera(-73.8, -7.6, 0.475, 26.75)
    Ws, bs, latent = fixture.make_decoder_weights()
    out = dict(K=K, R=R, T=T, H=H, W=W, latent=latent, weights_sha256=fixture.weights_sha256(Ws, bs), names=np.array(sorted(CASES)),
               **{k: np.float64(v) for k, v in BASE.items()})
    rsn = np.random.RandomState(99)
    dec = rh.build_reference_decoder(Ws, bs)
    dec_ns = [rh.build_reference_decoder([(Wl * (1 + 1e-7 * rsn.standard_normal(Wl.shape))).astype(np.float32) for Wl in Ws], bs) for _ in range(3)]
    for name in sorted(CASES):
        ckw, rkw = CASES[name]
        ckw = dict(BASE, **ckw)
        a = go.run(dec, latent, K, R, T, ckw, rkw, img_hw=(H, W))
        for k, v in a.items():
            out['%s.%s' % (name, k)] = v
        fl = dict(g_latent=0.0, g_R=0.0, g_T=0.0, flips=0, normal=0.0)
        unstable = np.zeros((H, W), bool)      # pixels whose depth / min-sdf the reference itself moves by more than 1e-5 under 1e-7 weight noise
        for dn in dec_ns:
            b = go.run(dn, latent, K, R, T, ckw, rkw, img_hw=(H, W))
            bothv = a['mask'].astype(bool) & b['mask'].astype(bool)
            unstable |= (np.abs(a['depth'] - b['depth']) > 1e-5) & bothv
            unstable |= np.abs(a['q'].reshape(H, W) - b['q'].reshape(H, W)) > 1e-5
            for k in ('g_latent', 'g_R', 'g_T'):
                fl[k] = max(fl[k], float(np.abs(a[k] - b[k]).max() / np.abs(a[k]).max()))
            fl['flips'] = max(fl['flips'], int((a['mask'] != b['mask']).sum()))
            if bothv.any():
                fl['normal'] = max(fl['normal'], float(np.percentile(np.abs(a['normal'] - b['normal'])[bothv], 99)))
        for k in ('g_latent', 'g_R', 'g_T'):
            out['%s.%s_floor_rel' % (name, k)] = fl[k]
        out['%s.unstable' % name] = unstable
        out['%s.flips_floor' % name] = fl['flips']
        out['%s.normal_p99_floor' % name] = fl['normal']
        out['%s.normal_scale' % name] = float(np.percentile(np.linalg.norm(a['normal'][a['mask'].astype(bool)], axis=-1), 99)) if a['mask'].any() else 1.0
        print(name, 'unstable px', int(unstable.sum()), 'valid', int(a['mask'].sum()), 'loss %.4f' % a['loss'], '|g_latent| %.3g' % np.abs(a['g_latent']).max(),
              'floors', {k: '%.1e' % out['%s.%s_floor_rel' % (name, k)] for k in ('g_latent', 'g_R', 'g_T')}, flush=True)
    # the two four-level cases share their coarse levels (the same march up to the fine level): a coarse ray that the reference stops one step
    # earlier under weight noise in either draw set moves the same 2 x 2 children in both -- their unstable pixels are the union
    pyr4 = [n for n in sorted(CASES) if CASES[n][0].get('scale_list') == PYR4['scale_list']]
    u = np.any([out[n + '.unstable'] for n in pyr4], axis=0)
    for n in pyr4:
        out[n + '.unstable'] = u
    np.savez_compressed(os.path.join(OUT, 'g30_short_fine_break.npz'), **out)
    print('g30 done')


if __name__ == '__main__':
    main()
