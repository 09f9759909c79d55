"""BP-SI on MI355X: binary min-sum BP with stabilizer inactivation as the post-processor of its own failures.

du Crest, Mhalla, Savin, "Stabilizer inactivation for message-passing decoding of quantum LDPC codes" (2022).  BP on a degenerate code
fails because it cannot choose between errors that differ by a stabilizer; so the least reliable stabilizer generator is taken, its few
bits are erased, BP runs again on the rest and the erased bits are filled in from a linear system of a handful of unknowns.  The
algorithm is stated at `fgnn_si_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_si.hip: one launch, the messages,
posteriors, group scores and marks of a codeword in LDS throughout.  Like Relay-BP and BP-GDG it needs no training and inverts no big
matrix: the one elimination per group (a few rows and columns) is done once, on the host, when the graph is first used.

The decoder works on a pair of matrices: the parity-check matrix and the matrix whose rows are the groups to inactivate.  For the Z
errors of a CSS code that is (hx, hz); for the X errors (hz, hx).
"""
import types

import numpy as np
import torch

from ._frontend import ShardedModel, bsc_logit, depolarizing_llr
from ._lib import ROWS_LX, ROWS_LZ
from .relay import RelayBPDecoder


def _dense(mat, what):
    mat = np.asarray(mat.toarray() if hasattr(mat, "toarray") else mat)
    if mat.ndim != 2 or not np.array_equal(mat, mat.astype(bool)):
        raise AssertionError(f'{what} must be a binary matrix.')
    return mat


def _si_graph(pcm, group_pcm, logical_pcm, device):
    """The graph of one binary decoder with groups: side 0 = pcm, side 1 = group_pcm, ``logical_pcm`` (or one zero row) as both
    residual row sets."""
    from .graph import TannerGraph
    pcm, group_pcm = np.asarray(pcm).astype(np.int64), np.asarray(group_pcm).astype(np.int64)
    n = pcm.shape[1]
    lp = np.zeros((1, n), np.int64) if logical_pcm is None else np.asarray(logical_pcm).astype(np.int64)
    zero = np.zeros((1, n), np.int64)
    code = types.SimpleNamespace(hx=pcm, hz=group_pcm, hx_perp=lp, hz_perp=lp, lx=zero, lz=zero)
    return TannerGraph(code, stage_one=True, device=device)


class SIDecoder:
    """``SIDecoder(pcm, group_pcm, num_iter=64, si_iter=32, max_groups=10, normalization_factor=0.8)``.  Min-sum BP on ``pcm`` runs up
    to ``num_iter`` iterations.  Where it finds no solution, the rows of ``group_pcm`` are ranked by the sum of their bits' |posterior|
    and up to ``max_groups`` of them, least reliable first, are inactivated one at a time: BP restarts with the group's bits erased,
    runs up to ``si_iter`` iterations, and as soon as every check away from the group is satisfied the erased bits are solved for.  The
    first attempt whose system is solvable gives the estimate; a sample that no attempt rescues keeps plain BP's decision.  A group may
    hold 32 bits and touch 64 checks at the most.

    Call ``decoder((llr_ch[bs,n], syndrome[m,bs]))`` as ``RelayBPDecoder``: ``llr_ch`` are logits, the result is ``e_hat[bs,n]`` (0/1
    floats).  ``last_stats[bs,4]`` (int32) = solution found, the attempt that found it (0: plain BP), its iteration, its group (-1 for
    plain BP); without a solution (0, attempts made, 0, -1)."""

    def __init__(self, pcm, group_pcm, num_iter=64, si_iter=32, max_groups=10, normalization_factor=0.8, device=None, graph=None):
        pcm, group_pcm = _dense(pcm, "PC matrix"), _dense(group_pcm, "group matrix")
        if group_pcm.shape[1] != pcm.shape[1]:
            raise ValueError("pcm and group_pcm must have the same number of columns")
        for name, val in (("num_iter", num_iter), ("si_iter", si_iter)):
            if not isinstance(val, (int, np.integer)) or val < 1:
                raise ValueError(f"{name} must be a positive integer")
        if not isinstance(max_groups, (int, np.integer)) or max_groups < 0:
            raise ValueError("max_groups cannot be negative")
        self._pcm, self._group_pcm = pcm, group_pcm
        self.num_iter, self.si_iter, self.max_groups = int(num_iter), int(si_iter), int(max_groups)
        self.normalization_factor = float(normalization_factor)
        self.graph = graph if graph is not None else _si_graph(pcm, group_pcm, None, device)
        if (self.graph.n, self.graph.m_x, self.graph.m_z) != (pcm.shape[1], pcm.shape[0], group_pcm.shape[0]):
            raise ValueError("graph does not have pcm on side 0 and group_pcm on side 1")
        self._num_vns, self._num_cns = self.graph.n, self.graph.m_x
        self.last_stats = None

    pcm = property(lambda self: self._pcm)
    group_pcm = property(lambda self: self._group_pcm)
    num_cns = property(lambda self: self._num_cns)
    num_vns = property(lambda self: self._num_vns)

    def decode(self, synd, llr_ch=None, llr_const=0.0, B=None, index=None, nact=None, out=None):
        """Estimates and stats for syndromes [B, m] (uint8, device) under per-bit logits ``llr_ch`` [B, n] or one logit for every bit;
        ``index`` / ``nact`` / ``out`` as `TannerGraph.si_decode`."""
        hard, stats = self.graph.si_decode(synd, self.num_iter, self.si_iter, self.max_groups, self.normalization_factor, llr_ch=llr_ch,
                                           llr_const=llr_const, B=B, index=index, nact=nact, out=out)
        self.last_stats = stats
        return hard, stats

    __call__ = RelayBPDecoder.__call__
    call = __call__


class BP2_SI_Model(ShardedModel):
    """``BP2_SI_Model(pcm, group_pcm, logical_pcm, si_decoder)``; ``model(batch_size, p)`` → ``(s_hat[bs,m], ls_hat[bs,
    rows(logical_pcm)])``, shaped like ``BP2_GDG_Model``: BSC(p) noise, its syndrome, BP-SI.  ``s_hat = pcm·(noise xor estimate)`` is
    non-zero exactly on the samples for which no attempt found a solution, ``ls_hat = logical_pcm·(noise xor estimate)``.  After a call
    ``last_noise``, ``last_estimate`` (uint8 [bs,n]), ``last_stats`` (int32 [bs,4]) and ``last_num_unsolved`` describe that batch.
    Side 1 of the model's graph is the group matrix, so noise and residual go through side 0: its checks and its row set."""

    def __init__(self, pcm, group_pcm, logical_pcm, si_decoder, *, seed=0x5EED, rank=0, world_size=1):
        self.pcm, self.group_pcm, self.logical_pcm, self.si_decoder = pcm, group_pcm, logical_pcm, si_decoder
        self.graph = _si_graph(pcm, group_pcm, logical_pcm, si_decoder.graph.device)
        self._shard(seed, rank, world_size)
        self.last_noise = self.last_estimate = self.last_stats = None
        self.last_num_unsolved = 0

    def __call__(self, batch_size, ebno_db=None, **kw):
        p = float(kw.get("p", ebno_db))
        B, g, d = int(batch_size), self.graph, self.si_decoder
        noise = g.bsc_noise(self.seed, p, self._take(B), B)
        zeros = torch.zeros_like(noise)
        synd, _ = g.syndrome(zeros, noise)       # side 0 measures the second noise array
        noise_hat, stats = d.decode(synd, llr_const=bsc_logit(p), B=B)
        self.last_noise, self.last_estimate, self.last_stats = noise, noise_hat, stats
        self.last_num_unsolved = int((stats[:, 0] == 0).sum().item())
        s_hat, ls_hat, _ = g.residual(zeros, noise, zeros, noise_hat, want_arrays=True)
        return s_hat[:, g.m_z:].contiguous(), ls_hat[:, g.rows_hxp:].contiguous()

    call = __call__


class BP4_SI_Model(ShardedModel):
    """``BP4_SI_Model(code, bp4_decoder, si_decoder_z, si_decoder_x)``; ``model(batch_size, p)`` → ``(s_hat[bs, m_z+m_x], ls_hat[bs,
    rows(lz)+rows(lx)])``, built like ``BP4_LSD_Model``: depolarizing noise of rate ``p``, BP4 on every sample, the samples whose
    estimate misses a syndrome compacted and handed as an index list to BP-SI: ``si_decoder_z`` = ``SIDecoder(code.hx, code.hz)`` gives
    their ``z_hat`` from ``synd_x``, ``si_decoder_x`` = ``SIDecoder(code.hz, code.hx)`` their ``x_hat`` from ``synd_z``, each with the
    constant prior logit of a bit flipped with probability ``2p/3``.  On a listed sample each half is BP-SI's output: its solution, or
    without one its plain min-sum decision.  Unlike LSD, SI may leave a sample unsolved, so ``s_hat`` is the true residual syndrome
    ``[hz·xd ; hx·zd]``; ``ls_hat = [lz·xd ; lx·zd]``.  ``last_num_si`` counts the list, ``last_num_unsolved`` the listed samples with a
    half unsolved, ``last_stats`` [2, bs, 4] holds the SI stats of side 0 (hx, z_hat) and side 1 (hz, x_hat), (1, 0, 0, -1) on the
    samples BP4 solved."""

    def __init__(self, code, bp4_decoder, si_decoder_z, si_decoder_x, *, seed=0x5EED, rank=0, world_size=1):
        from .feedback_gnn import Pauli
        self.code, self.bp4_decoder, self.si_decoder_z, self.si_decoder_x = code, bp4_decoder, si_decoder_z, si_decoder_x
        self.graph = g = bp4_decoder.graph
        for d, m, what in ((si_decoder_z, g.m_x, "si_decoder_z decodes on code.hx"), (si_decoder_x, g.m_z, "si_decoder_x decodes on code.hz")):
            if (d.num_vns, d.num_cns) != (g.n, m):
                raise ValueError(what)
        self.channel = Pauli(g, seed=seed)
        self._shard(self.channel.seed, rank, world_size)
        self.last_num_si = self.last_num_unsolved = 0
        self.last_stats = None

    def decode(self, batch_size, p):
        B, g, d = int(batch_size), self.graph, self.bp4_decoder
        ex, ez = self.channel(B, float(p), self._take(B))
        sx, sz = g.syndrome(ex, ez)
        decode = g.bp4_decode_layered if getattr(d, "schedule", "flooding") == "layered" else g.bp4_decode
        out = decode(sx, sz, d.num_iter, d.cn_type, d.normalization_factor, llr_const=depolarizing_llr(p), want_logits=False)
        x_hat, z_hat = out["x_hat"], out["z_hat"]
        _, _, flags = g.residual(ex, ez, x_hat, z_hat, want_arrays=False)  # bit 0 = syndrome missed
        index, nact = g.compact(flags, 1)
        self.last_num_si, self.last_num_unsolved = nact, 0
        self.last_stats = stats = torch.zeros((2, B, 4), dtype=torch.int32, device=g.device)
        stats[:, :, 0], stats[:, :, 3] = 1, -1
        if nact:
            prior = bsc_logit(2.0 * float(p) / 3.0)
            self.si_decoder_z.decode(sx, llr_const=prior, index=index, nact=nact, out=(z_hat, stats[0]))
            self.si_decoder_x.decode(sz, llr_const=prior, index=index, nact=nact, out=(x_hat, stats[1]))
            self.last_num_unsolved = int((stats[:, :, 0] == 0).any(0).sum().item())
        return dict(noise_x=ex, noise_z=ez, x_hat=x_hat, z_hat=z_hat)

    def __call__(self, batch_size, ebno_db=None, **kw):
        o = self.decode(batch_size, kw.get("p", ebno_db))
        g = self.graph
        s_hat, _, _ = g.residual(o["noise_x"], o["noise_z"], o["x_hat"], o["z_hat"], want_arrays=True)
        ls_hat, _ = g.residual_rows(ROWS_LZ, ROWS_LX, o["noise_x"], o["noise_z"], o["x_hat"], o["z_hat"])
        return s_hat, ls_hat

    call = __call__
