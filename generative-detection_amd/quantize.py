"""VectorQuantizer: [UPSTREAM] taming.modules.vqvae.quantize.VectorQuantizer2 (what ldm's VQModel imports as VectorQuantizer) on the
fused search kernel of csrc/vq_f32.hip.  Constructor signature, `embedding.weight` and the return tuple are upstream's; upstream's
permute -> distance matrix -> argmin -> embedding lookup -> permute is one op here (ops.vq_quantize)."""
import torch
import torch.nn as nn

from . import ops


class VectorQuantizer(nn.Module):
    def __init__(self, n_e, e_dim, beta, remap=None, unknown_index="random", sane_index_shape=False, legacy=True):
        super().__init__()
        self.n_e = n_e
        self.e_dim = e_dim
        self.beta = beta
        self.legacy = legacy
        self.embedding = nn.Embedding(self.n_e, self.e_dim)
        self.embedding.weight.data.uniform_(-1.0 / self.n_e, 1.0 / self.n_e)
        self.remap = remap
        if self.remap is not None:
            raise NotImplementedError("VectorQuantizer(remap=%r): remapping needs a file of used indices and is not implemented "
                                      "(unknown_index=%r goes with it)" % (remap, unknown_index))
        self.re_embed = n_e
        self.sane_index_shape = sane_index_shape

    def forward(self, z, temp=None, rescale_logits=False, return_logits=False):
        assert temp is None or temp == 1.0, "Only for interface compatible with Gumbel"
        assert rescale_logits is False, "Only for interface compatible with Gumbel"
        assert return_logits is False, "Only for interface compatible with Gumbel"
        z_q, loss, min_encoding_indices = ops.vq_quantize(z, self.embedding.weight, self.beta, self.legacy)
        if self.sane_index_shape:
            min_encoding_indices = min_encoding_indices.reshape(z_q.shape[0], z_q.shape[2], z_q.shape[3])
        return z_q, loss, (None, None, min_encoding_indices)

    def get_codebook_entry(self, indices, shape):
        """shape = (batch, height, width, channel); returns [batch, channel, height, width].  With shape None, the codes as rows."""
        if shape is None:
            flat = indices.reshape(-1)
            return ops.vq_gather(flat, self.embedding.weight, (flat.numel(), 1, 1, self.e_dim)).reshape(flat.numel(), self.e_dim)
        return ops.vq_gather(indices, self.embedding.weight, shape)
