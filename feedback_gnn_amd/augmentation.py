"""Augmented BP4 on MI355X: the fourth hand-written baseline the learned feedback of the GNN (arXiv 2310.17758) is measured against.

Augmentation is Rigby, Olivier and Jarvis, "Modified belief propagation decoders for quantum low-density parity-check codes" (Phys.
Rev. A 100, 012330, 2019): when BP4 has run its iterations without a solution, a random fraction of the check rows is written into the
matrix a second time and BP4 runs again, with fresh draws until an estimate reproduces the syndrome.  The algorithm is stated at
`fgnn_bp4aug_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_bp4aug.hip: one launch, all attempts of a codeword with
its messages, decisions and duplicate marks in LDS throughout.  The augmented matrix is never built: a qubit adds the message of a
duplicated check twice.  No training, no matrix inversion, no change to the check rule.
"""
import numpy as np

from ._frontend import CodeDecoder, DepolarizingBP4Model
from ._lib import CN_TYPES


class BP4AugmentedDecoder(CodeDecoder):
    """``BP4AugmentedDecoder(code, pre_iter=32, attempt_iter=32, max_attempts=40, density=0.1, restart=True, cn_type="minsum",
    normalization_factor=0.8, seed=0x5EED)``.  BP4 runs up to ``pre_iter`` iterations; while no estimate reproduces both syndromes, up
    to ``max_attempts`` times, every check row is duplicated with probability ``density`` and BP4 runs up to ``attempt_iter`` iterations
    on that code, from zero messages (``restart=True``, what the paper does) or from the messages it has.

    Call ``decoder((llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs]))`` as ``QLDPCBPDecoder``: the result is
    ``(x_hat, z_hat)`` [bs,n] in its dtypes (int64 and float64).  ``last_stats[bs,4]`` (int32) = solution found, draws made,
    iterations run, and the iteration within its attempt of the last test.  The marks are drawn from the Philox stream of ``seed`` at
    the sample indices ``first_sample`` .. of ``decode``, apart from the channel noise of the same seed."""

    def __init__(self, code, pre_iter=32, attempt_iter=32, max_attempts=40, density=0.1, restart=True, cn_type="minsum",
                 normalization_factor=0.8, seed=0x5EED, device=None, graph=None):
        for name, val in (("pre_iter", pre_iter), ("attempt_iter", attempt_iter)):
            if not isinstance(val, (int, np.integer)) or val < 1:
                raise ValueError(f"{name} must be a positive integer")
        if not isinstance(max_attempts, (int, np.integer)) or not 0 <= max_attempts <= 65535:
            raise ValueError("max_attempts must be an integer in 0 .. 65535")
        if not (np.isfinite(float(density)) and 0.0 <= float(density) <= 1.0):
            raise ValueError("density must be finite and in [0, 1]")
        if cn_type not in CN_TYPES:
            raise ValueError("Unknown node type.")
        self.pre_iter, self.attempt_iter, self.max_attempts = int(pre_iter), int(attempt_iter), int(max_attempts)
        self.density, self.restart, self.seed = float(density), bool(restart), int(seed)
        self.cn_type, self.normalization_factor = cn_type, float(normalization_factor)
        self._attach(code, graph, device)

    def decode(self, synd_x, synd_z, llr_ch=None, llr_const=0.0, first_sample=0, seed=None):
        """Estimates and stats for syndromes [B, m_x] / [B, m_z] (uint8, device) under ``llr_ch`` [B, 3, n] or one LLR for everything;
        row b is decoded as global sample ``first_sample + b`` of the stream of ``seed`` (None: the decoder's)."""
        x_hat, z_hat, stats = self.graph.bp4aug_decode(synd_x, synd_z, self.pre_iter, self.attempt_iter, self.max_attempts, self.density,
                                                       self.cn_type, self.normalization_factor, restart=self.restart,
                                                       seed=self.seed if seed is None else seed, first_sample=first_sample,
                                                       llr_ch=llr_ch, llr_const=llr_const)
        self.last_stats = stats
        return x_hat, z_hat, stats


class BP4_Augmented_Model(DepolarizingBP4Model):
    """``BP4_Augmented_Model(code, decoder, p0=None)``; ``model(batch_size, p)`` → ``(s_hat[bs, m_z+m_x], ls_hat[bs,
    rows(hx_perp)+rows(hz_perp)])``, shaped like ``BP4_Feedback_Model``: depolarizing noise of rate ``p``, its two syndromes, augmented
    BP4 under the prior ``log(3(1-p0)/p0)`` (``p0=None``: of ``p`` itself).  The marks use the model's ``seed`` and the batch's global
    sample indices, so a shard decodes its samples exactly as a single process would.  ``s_hat`` is non-zero exactly on the samples for
    which no solution was found.  After a call ``last_noise_x``, ``last_noise_z``, ``last_x_hat``, ``last_z_hat`` (uint8 [bs,n]),
    ``last_stats`` (int32 [bs,4]) and ``last_num_unsolved`` describe that batch.  ``rank`` / ``world_size`` shard the sample stream."""

    def _decode(self, sx, sz, llr_const, first):
        return self.decoder.decode(sx, sz, llr_const=llr_const, first_sample=first, seed=self.seed)
