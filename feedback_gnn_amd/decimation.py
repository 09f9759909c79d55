"""BP4 with guided decimation (BP4-GD) on MI355X: quaternary BP that, when it stalls, fixes its most reliable undecided qubit and goes on.

Yao, Abu Laban, Haeger, Amat, Pfister, "Belief propagation decoding of quantum LDPC codes with guided decimation" (2023), quaternary
variant.  The algorithm is stated at `fgnn_bp4gd_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_bp4gd.hip: one
launch, the messages, decisions and fix marks of a codeword in LDS throughout.  Like Relay-BP it needs no training and no matrix
inversion.
"""
import numpy as np

from ._frontend import CodeDecoder, DepolarizingBP4Model, alias
from ._lib import CN_TYPES


class BP4GDDecoder(CodeDecoder):
    """``BP4GDDecoder(code, pre_iter=32, round_iter=4, max_rounds=None, decim_llr=25.0, cn_type="minsum", normalization_factor=0.8)``.
    BP4 runs up to ``pre_iter`` iterations; while no estimate reproduces both syndromes, up to ``max_rounds`` times (``None``: n), the
    free qubit whose decision leads its runner-up by the largest margin is fixed to that decision (its LLRs become ``-decim_llr`` for the
    decided Pauli and 0 for the others, or ``+decim_llr`` on all three for the identity) and BP4 runs up to ``round_iter`` iterations
    more from the messages it has.

    Call ``decoder((llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs]))`` as ``QLDPCBPDecoder``: the result is
    ``(x_hat, z_hat)`` [bs,n] in its dtypes (int64 and float64).  ``last_stats[bs,4]`` (int32) = solution found, qubits fixed, iterations
    run, and the iteration within its round of the last test."""

    def __init__(self, code, pre_iter=32, round_iter=4, max_rounds=None, decim_llr=25.0, cn_type="minsum", normalization_factor=0.8,
                 device=None, graph=None):
        for name, val in (("pre_iter", pre_iter), ("round_iter", round_iter)):
            if not isinstance(val, (int, np.integer)) or val < 1:
                raise ValueError(f"{name} must be a positive integer")
        if max_rounds is not None and (not isinstance(max_rounds, (int, np.integer)) or max_rounds < 0):
            raise ValueError("max_rounds cannot be negative")
        if not float(decim_llr) > 0:
            raise ValueError("decim_llr must be positive")
        if cn_type not in CN_TYPES:
            raise ValueError("Unknown node type.")
        self.pre_iter, self.round_iter = int(pre_iter), int(round_iter)
        self.decim_llr, self.cn_type, self.normalization_factor = float(decim_llr), cn_type, float(normalization_factor)
        self._attach(code, graph, device)
        self.max_rounds = self._num_vns if max_rounds is None else int(max_rounds)

    def decode(self, synd_x, synd_z, llr_ch=None, llr_const=0.0):
        """Estimates and stats for syndromes [B, m_x] / [B, m_z] (uint8, device) under ``llr_ch`` [B, 3, n] or one LLR for everything."""
        x_hat, z_hat, stats = self.graph.bp4gd_decode(synd_x, synd_z, self.pre_iter, self.round_iter, self.max_rounds, self.decim_llr,
                                                      self.cn_type, self.normalization_factor, llr_ch=llr_ch, llr_const=llr_const)
        self.last_stats = stats
        return x_hat, z_hat, stats


class BP4_GD_Model(DepolarizingBP4Model):
    """``BP4_GD_Model(code, gd_decoder, p0=None)``; ``model(batch_size, p)`` → ``(s_hat[bs, m_z+m_x], ls_hat[bs,
    rows(hx_perp)+rows(hz_perp)])``, shaped like ``BP4_Relay_Model``: depolarizing noise of rate ``p``, its two syndromes, BP4-GD with
    the prior ``log(3(1-p0)/p0)`` (``p0=None``: of ``p`` itself).  ``s_hat`` is non-zero exactly on the samples for which no solution
    was found.  After a call ``last_noise_x``, ``last_noise_z``, ``last_x_hat``, ``last_z_hat`` (uint8 [bs,n]), ``last_stats`` (int32
    [bs,4]) and ``last_num_unsolved`` describe that batch.  ``rank`` / ``world_size`` shard the sample stream."""

    def __init__(self, code, gd_decoder, p0=None, *, seed=0x5EED, rank=0, world_size=1):
        super().__init__(code, gd_decoder, p0, seed=seed, rank=rank, world_size=world_size)

    gd_decoder = alias("decoder")
