"""TEST INFRASTRUCTURE -- the decoder-path term of the autograd normals' backward, restated twice in torch (float64 by default).

render_normal differentiates the decoder with create_graph=True (core/utils/decoder_utils.py:76-92, core/sdfrenderer/renderer.py:880-910 of
the reference), so a loss on the normal image reaches the shape code and the camera through the decoder a second time. Given the surface
depths and the mask of a render (the march itself is detached there: has_zdepth_grad=False, renderer.py:895), the term is a function of
(code, R, T) alone:

    definition(...)   the torch Decoder, torch.autograd.grad(create_graph=True) on the points, a second backward to code and camera;
    closed_form(...)  a ReLU decoder is piecewise linear in (code, x): with f = tanh(u) the raw normal is h = 3 1[|f| <= clamp] (1 - f^2) grad_x u
                      and grad_x u is locally constant, so the whole second-order path is one upstream scalar on f per surface sample,
                      g_f = -2 f (g . h) / (1 - f^2), g = dL/dh, fed to the ordinary first-order backward at the surface point.

Both return dict(g_latent (1, C), g_R (3, 3), g_T (3,), g_R_product (3, 3), n): g_R is the decoder-path share alone, g_R_product the share
of the explicit `R @ normal` product (renderer.py:978) that every build has always returned; the reference's g_R is their sum.
"""
import numpy as np
import torch

# Residual of definition() in float64 against golden G27 (max abs, the reference's float32 gradients), on the CPU oracle's render of G27's
# configuration -- recorded because the golden's noise floors (the reference under 1e-7 relative weight noise) sit below the distance
# between a float64 restatement and a float32 reference on some components: where 2 x this residual exceeds 2 x the floor, it is the bar
# (bar() below). Measured with tests/test_normal_decoder_grad_host.py, never taken from the HIP path.
RESIDUAL_A = {
    'f1_recursive_raw': dict(g_latent=4.594e-07, g_R=1.788e-02, g_T=1.043e-05),
    'f1_pyramid_recursive_raw': dict(g_latent=5.596e-07, g_R=2.376e-03, g_T=1.835e-05),
    'f2_recursive_raw': dict(g_latent=1.069e-05, g_R=4.902e-02, g_T=7.814e-05),
    'f2_pyramid_recursive_raw': dict(g_latent=1.579e-06, g_R=4.902e-02, g_T=2.226e-05),
}


def bar(g, key, k):
    """Bar of gradient k of G27 case `key` (g: the loaded golden): the project's bar for goldens, 2 x the recorded noise floor, or
    2 x the definition's own residual against the golden where that is larger."""
    return max(2.0 * float(g['%s.%s_floor' % (key, k)]), 2.0 * RESIDUAL_A.get(key, {}).get(k, 0.0))


DEFAULT_M = np.array([[1., 0., 0.], [0., 0., -1.], [0., 1., 0.]])


def module(Ws, bs, dtype=torch.float64):
    """The torch Decoder (core/graph/deep_sdf_decoder.py) holding the weights (Ws, bs), on the CPU."""
    from core.graph.deep_sdf_decoder import Decoder
    from distr import decoder_pack
    dec = Decoder(decoder_pack.latent_size_of(Ws), [512] * 8, norm_layers=(), latent_in=[4])
    dec.load_state_dict({('lin%d.%s' % (l, n)): torch.from_numpy(np.asarray(a, np.float32)) for l, (W_, b) in enumerate(zip(Ws, bs))
                         for n, a in (('weight', W_), ('bias', b))})
    return dec.to(dtype).eval()


class Scene(object):
    """Constants of one view: intrinsics, matrices, the valid pixels with their surface depths, the upstream gradient of the normal image."""

    def __init__(self, H, W, K, zdepth, mask, g_normal, clamp_dist=0.1, normalize=False, transform_matrix=None, use_transform=True,
                 dtype=torch.float64):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        self.dtype = dtype
        self.K_inv = t(np.linalg.inv(np.asarray(K, np.float64)).astype(np.float32))            # float32(inv(K)), renderer.py:161-164
        Mn = np.asarray(DEFAULT_M if transform_matrix is None else transform_matrix, np.float32)
        self.Mn = t(Mn)                                                                        # the normals' matrix (renderer.py:899)
        self.M = t(Mn if use_transform else np.eye(3, dtype=np.float32))                       # the points' (inverse) matrix (:895)
        pix = np.nonzero(np.asarray(mask).reshape(-1))[0]
        self.pix = torch.from_numpy(pix)
        self.z = t(np.asarray(zdepth, np.float32).reshape(-1)[pix])
        self.w = t(np.asarray(g_normal, np.float32).reshape(-1, 3)[pix])                       # (n, 3) = dL / d normal[pix]
        px, py = (pix % W).astype(np.float32), (pix // W).astype(np.float32)
        self.homo = t(np.stack([px, py, np.ones_like(px)], 0))                                 # (3, n)
        self.cd, self.normalize = float(clamp_dist), bool(normalize)
        self.n = int(pix.size)

    def points(self, R, T):
        """(n, 3) surface points in the decoder's frame, differentiable in the camera; the depths are constants."""
        rays = R.t() @ (self.K_inv @ self.homo)
        rays = rays / (torch.norm(rays, p=2, dim=0, keepdim=True) + 1e-12)
        cam = -(R.t() @ T)
        return (self.M.t() @ (cam[:, None] + rays * self.z[None])).t()

    def pulled_back(self, R):
        """g = dL/dh (n, 3): the upstream gradient through the x flip, R and the normals' matrix."""
        go = self.w * torch.tensor([-1., 1., 1.], dtype=self.dtype)
        return (self.Mn.t() @ (R.t() @ go.t())).t()


def _inputs(latent, R, T, dtype):
    mk = lambda a, shape: torch.from_numpy(np.asarray(a, np.float32)).to(dtype).reshape(shape).clone().requires_grad_(True)
    return mk(latent, (1, -1)), mk(R, (3, 3)), mk(T, (3,))


def _result(lat, R, T, g_R_product, n):
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.detach().numpy().copy()
    return dict(g_latent=z(lat), g_R=z(R), g_T=z(T), g_R_product=g_R_product, n=n)


def _zero(latent, n=0):
    return dict(g_latent=np.zeros((1, np.asarray(latent).size)), g_R=np.zeros((3, 3)), g_T=np.zeros(3), g_R_product=np.zeros((3, 3)), n=n)


def _raw_normal(dec, S, lat, pts, create_graph):
    """h (n, 3) = 3 x d clamp(f) / d points (the factor 3: grad_outputs of the points' shape, decoder_utils.py:84), and f (n,)."""
    f = dec(torch.cat([lat.expand(pts.shape[0], -1), pts], 1))
    fc = torch.clamp(f, -S.cd, S.cd)
    h, = torch.autograd.grad(fc, pts, grad_outputs=3.0 * torch.ones_like(fc), create_graph=create_graph)
    return h, f.reshape(-1)


def _product_share(S, R, h):
    """Gradient of sum(flip(R Mn n) * w) with respect to R with the normals n held constant (renderer.py:978)."""
    n = h.detach()
    if S.normalize:
        n = n / (torch.norm(n, p=2, dim=1, keepdim=True) + 1e-12)
    Rp = R.detach().clone().requires_grad_(True)
    o = (Rp @ (S.Mn @ n.t())).t() * torch.tensor([-1., 1., 1.], dtype=S.dtype)
    (o * S.w).sum().backward()
    return Rp.grad.numpy().copy()


def definition(dec, S, latent, R, T):
    """(a) The term as the reference computes it: double backward through the decoder."""
    if S.n == 0:
        return _zero(latent)
    lat, Rt, Tt = _inputs(latent, R, T, S.dtype)
    pts = S.points(Rt, Tt)
    h, _ = _raw_normal(dec, S, lat, pts, True)
    n = h / (torch.norm(h, p=2, dim=1, keepdim=True) + 1e-12) if S.normalize else h
    o = (Rt.detach() @ (S.Mn @ n.t())).t() * torch.tensor([-1., 1., 1.], dtype=S.dtype)      # R detached: the decoder path alone
    (o * S.w).sum().backward()
    return _result(lat, Rt, Tt, _product_share(S, Rt, h), S.n)


def closed_form(dec, S, latent, R, T):
    """(b) g_f = -2 f (g . h) / (1 - f^2) into the first-order backward of the decoder at the surface points; zero for unit normals."""
    if S.n == 0:
        return _zero(latent)
    lat, Rt, Tt = _inputs(latent, R, T, S.dtype)
    p0 = S.points(Rt, Tt).detach().requires_grad_(True)
    h, f = _raw_normal(dec, S, lat.detach(), p0, False)
    h, f = h.detach(), f.detach()
    prod = _product_share(S, Rt, h)
    if S.normalize:
        return dict(_zero(latent, S.n), g_R_product=prod)
    gh = (S.pulled_back(Rt.detach()) * h).sum(1)
    g_f = torch.where(f.abs() <= S.cd, -2.0 * f * gh / (1.0 - f * f), torch.zeros_like(f))
    pts = S.points(Rt, Tt)
    f1 = dec(torch.cat([lat.expand(pts.shape[0], -1), pts], 1)).reshape(-1)
    (f1 * g_f).sum().backward()
    return _result(lat, Rt, Tt, prod, S.n)
