"""BP4 with guided decimation (BP4-GD) on MI355X: quaternary BP that, when it stalls, fixes its most reliable undecided qubit and goes on.

Yao, Abu Laban, Haeger, Amat, Pfister, "Belief propagation decoding of quantum LDPC codes with guided decimation" (2023), quaternary
variant.  The algorithm is stated at `fgnn_bp4gd_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_bp4gd.hip: one
launch, the messages, decisions and fix marks of a codeword in LDS throughout.  Like Relay-BP it needs no training and no matrix
inversion.

BP-GDG (`GDGDecoder`, `BP2_GDG_Model`) is decimation on the binary decoder, on any parity-check matrix with per-bit priors: guided
decimation guessing (Gong, Cammerer, Renes, "Toward low-latency iterative decoding of QLDPC codes under circuit-level noise", 2024).
The least reliable bit is decimated, for the first ``depth`` decimations both values are tried, each of the 2**depth paths then goes on
greedily and the lowest-weight solution wins.  Stated at `fgnn_gdg_decode` in include/fgnn.h; the kernels are in
feedback_gnn_amd/csrc/fgnn_gdg.hip: a path is a codeword of its own, LDS-resident, and a small second kernel selects.
"""
import numpy as np
import torch

from ._frontend import CodeDecoder, DepolarizingBP4Model, ShardedModel, alias, bsc_logit
from ._lib import CN_TYPES, GDG_MAX_DEPTH, GDG_TAILS
from .decoding import _binary_graph
from .relay import RelayBPDecoder


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


class GDGDecoder:
    """``GDGDecoder(pcm, pre_iter=32, round_iter=4, max_rounds=None, depth=3, tail="least", decim_llr=25.0, normalization_factor=0.8,
    prefilter=True)``.  Min-sum BP runs up to ``pre_iter`` iterations; while no estimate reproduces the syndrome, up to ``max_rounds``
    times (``None``: n), a free bit is fixed (its prior becomes ``+-decim_llr``) and BP runs up to ``round_iter`` iterations more from the
    messages it has.  The first ``depth`` fixes take the least reliable bit and try both values, which makes ``2**depth`` paths; the
    later ones take the least (``tail="least"``) or most (``"most"``) reliable bit at its current decision.  The solution of lowest
    weight among the paths is the estimate.  ``depth=0, tail="most"`` is binary BPGD.

    With ``prefilter`` one launch of plain BP (depth 0, no fixes) decodes the whole batch first and the tree runs on the unsolved
    samples only: the same estimates bit for bit, and easy samples do not pay ``2**depth`` times.

    Call ``decoder((llr_ch[bs,n], syndrome[m,bs]))`` as ``RelayBPDecoder``: ``llr_ch`` are logits, the result is ``e_hat[bs,n]`` (0/1
    floats).  ``last_stats[bs,4]`` (int32) = paths that found a solution (with ``prefilter``: 1 on the samples plain BP solved), weight
    of the estimate (0 when none found), its path, the bits fixed on that path."""

    def __init__(self, pcm, pre_iter=32, round_iter=4, max_rounds=None, depth=3, tail="least", decim_llr=25.0, normalization_factor=0.8,
                 prefilter=True, device=None, graph=None):
        pcm = np.asarray(pcm.toarray() if hasattr(pcm, "toarray") else pcm)
        if not np.array_equal(pcm, pcm.astype(bool)):
            raise AssertionError('PC matrix must be binary.')
        for name, val in (("pre_iter", pre_iter), ("round_iter", round_iter)):
            if not isinstance(val, (int, np.integer)) or val < 1:
                raise ValueError(f"{name} must be a positive integer")
        if max_rounds is not None and (not isinstance(max_rounds, (int, np.integer)) or max_rounds < 0):
            raise ValueError("max_rounds cannot be negative")
        if not isinstance(depth, (int, np.integer)) or not 0 <= depth <= GDG_MAX_DEPTH:
            raise ValueError(f"depth must be an integer in 0 .. {GDG_MAX_DEPTH}")
        if tail not in GDG_TAILS:
            raise ValueError('tail must be "least" or "most"')
        if not float(decim_llr) > 0:
            raise ValueError("decim_llr must be positive")
        self._pcm = pcm
        self.pre_iter, self.round_iter, self.depth, self.tail = int(pre_iter), int(round_iter), int(depth), tail
        self.decim_llr, self.normalization_factor, self.prefilter = float(decim_llr), float(normalization_factor), bool(prefilter)
        self.graph = graph if graph is not None else _binary_graph(pcm, None, device)
        self._num_vns, self._num_cns = self.graph.n, self.graph.m_x
        self.max_rounds = self._num_vns if max_rounds is None else int(max_rounds)
        self.last_stats = None

    pcm = property(lambda self: self._pcm)
    num_cns = property(lambda self: self._num_cns)
    num_vns = property(lambda self: self._num_vns)

    def decode(self, synd, llr_ch=None, llr_const=0.0, B=None):
        """Estimates and stats for syndromes [B, m] (uint8, device) under per-bit logits ``llr_ch`` [B, n] or one logit for every bit."""
        g = self.graph
        args = (self.pre_iter, self.round_iter)
        kw = dict(tail=self.tail, decim_llr=self.decim_llr, factor=self.normalization_factor, llr_ch=llr_ch, llr_const=llr_const, B=B)
        if self.prefilter and (self.depth > 0 or self.max_rounds > 0):
            hard, stats = g.gdg_decode(synd, *args, 0, 0, **kw)
            index, nact = g.compact((stats[:, 0] == 0).to(torch.uint8))
            if nact:
                g.gdg_decode(synd, *args, self.max_rounds, self.depth, index=index, nact=nact, out=(hard, stats), **kw)
        else:
            hard, stats = g.gdg_decode(synd, *args, self.max_rounds, self.depth, **kw)
        self.last_stats = stats
        return hard, stats

    __call__ = RelayBPDecoder.__call__
    call = __call__


class BP2_GDG_Model(ShardedModel):
    """``BP2_GDG_Model(pcm, logical_pcm, gdg_decoder)``; ``model(batch_size, p)`` → ``(s_hat[bs,m], ls_hat[bs,rows(logical_pcm)])``,
    shaped like ``BP2_Relay_Model``: BSC(p) noise, its syndrome, BP-GDG.  ``s_hat = pcm·(noise xor estimate)`` is non-zero exactly on the
    samples for which no path found a solution, ``ls_hat = logical_pcm·(noise xor estimate)``.  After a call ``last_noise``,
    ``last_estimate`` (uint8 [bs,n]), ``last_stats`` (int32 [bs,4]) and ``last_num_unsolved`` describe that batch."""

    def __init__(self, pcm, logical_pcm, gdg_decoder, *, seed=0x5EED, rank=0, world_size=1):
        self.pcm, self.logical_pcm, self.gdg_decoder = pcm, logical_pcm, gdg_decoder
        self.graph = _binary_graph(pcm, logical_pcm, gdg_decoder.graph.device)
        self._shard(seed, rank, world_size)
        self.last_noise = self.last_estimate = self.last_stats = None
        self.last_num_unsolved = 0

    def __call__(self, batch_size, ebno_db=None, **kw):
        p = float(kw.get("p", ebno_db))
        B, g = int(batch_size), self.graph
        noise = g.bsc_noise(self.seed, p, self._take(B), B)
        zeros = torch.zeros_like(noise)
        synd, _ = g.syndrome(zeros, noise)
        noise_hat, stats = self.gdg_decoder.decode(synd, llr_const=bsc_logit(p), B=B)
        self.last_noise, self.last_estimate, self.last_stats = noise, noise_hat, stats
        self.last_num_unsolved = int((stats[:, 0] == 0).sum().item())
        s_hat, ls_hat, _ = g.residual(noise, zeros, noise_hat, zeros, want_arrays=True)
        return s_hat[:, :g.m_z].contiguous(), ls_hat[:, :g.rows_hxp].contiguous()

    call = __call__
