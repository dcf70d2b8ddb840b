"""DeepSDF decoder module (architecture of facebookresearch/DeepSDF as used by the reference,
core/graph/deep_sdf_decoder.py:18-111). Holds parameters with the reference's state-dict keys
(lin{l}.weight / .bias, or .weight_g / .weight_v under weight_norm) so checkpoints load unchanged;
`inference` is a plain PyTorch evaluation used for validation only -- the renderer never calls it,
it packs the parameters for the MFMA kernels (distr.decoder_pack). `forward_train` is the reference's training forward
(deep_sdf_decoder.py:114-133) on the layer-wise GPU path (decode_sdf_train)."""
import torch
import torch.nn as nn


def threshold_min_max(values, lower, upper):
    """values limited to [lower, upper], element-wise with broadcasting (the name the reference's training loop knows)"""
    return torch.minimum(torch.maximum(values, lower), upper)


class Decoder(nn.Module):
    def __init__(self, latent_size, dims, last_dim=1, dropout=None, dropout_prob=0.0, norm_layers=(), latent_in=(),
                 weight_norm=False, xyz_in_all=None, use_tanh=False, latent_dropout=False):
        super(Decoder, self).__init__()
        widths = [latent_size + 3] + list(dims) + [last_dim]
        self.num_layers = len(widths)
        self.norm_layers, self.latent_in = norm_layers, latent_in
        self.latent_dropout, self.xyz_in_all = latent_dropout, xyz_in_all
        self.weight_norm, self.use_tanh = weight_norm, use_tanh
        self.dropout, self.dropout_prob = dropout, dropout_prob
        for l in range(self.num_layers - 1):
            n_out = widths[l + 1]
            if (l + 1) in latent_in:
                n_out -= widths[0]                      # room for the re-injected [latent|xyz]
            elif xyz_in_all and l != self.num_layers - 2:
                n_out -= 3
            lin = nn.Linear(widths[l], n_out)
            if weight_norm and l in norm_layers:
                lin = nn.utils.weight_norm(lin)
            setattr(self, 'lin%d' % l, lin)
            if (not weight_norm) and norm_layers is not None and l in norm_layers:
                setattr(self, 'bn%d' % l, nn.LayerNorm(n_out))
        self.th = nn.Tanh()

    def inference(self, inp):
        xyz = inp[:, -3:]
        if inp.shape[1] > 3 and self.latent_dropout:        # deep_sdf_decoder.py:84-89 (the identity in eval mode)
            inp = torch.cat([nn.functional.dropout(inp[:, :-3], p=0.2, training=self.training), xyz], 1)
        x = inp
        last = self.num_layers - 2
        for l in range(self.num_layers - 1):
            if l in self.latent_in:
                x = torch.cat([x, inp], 1)
            elif l != 0 and self.xyz_in_all:
                x = torch.cat([x, xyz], 1)
            x = getattr(self, 'lin%d' % l)(x)
            if l == last and self.use_tanh:
                x = torch.tanh(x)
            if l < last:
                if hasattr(self, 'bn%d' % l):
                    x = getattr(self, 'bn%d' % l)(x)
                x = torch.relu(x)
                if self.dropout is not None and l in self.dropout:
                    x = nn.functional.dropout(x, p=self.dropout_prob, training=self.training)
        return self.th(x)

    forward = inference

    def forward_train(self, sdf_data, lat_vecs_idx, min_vec, max_vec, enforce_minmax=True, dropout_seed=None):
        """The reference's training step (its `forward`, deep_sdf_decoder.py:114-133): sdf_data (B, S, 4) = xyz and the target sdf of
        S samples of B scenes, lat_vecs_idx (B, C) one code per scene -> (pred_sdf (B*S, 1), loss_l1 (B*S,), loss_l2_size (B,)),
        differentiable w.r.t. the codes and this module's parameters (decode_sdf_train with clamp_dist=None; the min/max clamp, the
        L1 loss and the code regulariser in torch). In training mode a decoder with dropout needs `dropout_seed`
        (distr.functions.draw_dropout_seed()): the mask of DESIGN.md section 8g, segment = scene index."""
        from core.utils.decoder_utils import decode_sdf_train
        B, S = sdf_data.shape[0], sdf_data.shape[1]
        flat = sdf_data.reshape(-1, 4)
        sdf_gt = flat[:, 3].unsqueeze(1)
        pred_sdf = decode_sdf_train(self, lat_vecs_idx, flat[:, 0:3].detach().reshape(B, S, 3), clamp_dist=None, dropout_seed=dropout_seed).reshape(-1, 1)
        if enforce_minmax:
            sdf_gt = threshold_min_max(sdf_gt, min_vec, max_vec)
            pred_sdf = threshold_min_max(pred_sdf, min_vec, max_vec)
        loss_l1 = torch.abs(pred_sdf - sdf_gt).squeeze(1)
        loss_l2_size = (lat_vecs_idx * lat_vecs_idx).mean(dim=1)       # the code regulariser, one value per scene
        return pred_sdf, loss_l1, loss_l2_size
