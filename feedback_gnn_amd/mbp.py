"""BP4 with message-strength control on MI355X: MBP4 and its adaptive form AMBP4 (Kuo, Lai, "Exploiting degeneracy in belief
propagation decoding of quantum codes", npj Quantum Information, 2022), flooding schedule.

A qubit's belief is formed from its incoming check messages scaled by ``1 / alpha``, while the message it sends back to a check has
that check's own contribution removed at full strength (the inhibition term); ``alpha < 1`` breaks the symmetric stalls that
degenerate codes cause.  AMBP4 tries a descending list of alphas and keeps the first whose estimate reproduces both syndromes.  The
algorithm is stated at `fgnn_mbp4_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_mbp4.hip: one launch, all
alphas of a codeword with its messages and decisions in LDS throughout.  It needs no training, no random numbers and no matrix
inversion.
"""
import numpy as np
import torch

from ._lib import CN_TYPES

ALPHA_DEFAULTS = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5)
MAX_ALPHAS = 64


def mbp4_tables(alphas, base):
    """``(factor, own)`` float32 arrays of `fgnn_mbp4_decode` for Kuo-Lai's MBP4: ``own[a] = float32(alpha_a)`` and ``factor[a] =
    float32(base) / float32(alpha_a)``, one IEEE float32 division."""
    own = np.asarray(alphas, dtype=np.float32).reshape(-1)
    factor = (np.float32(base) / own).astype(np.float32)
    return factor, own


class AMBP4Decoder:
    """``AMBP4Decoder(code, alphas=None, num_iter=64, cn_type="minsum", factor=0.8, restart=True)``.  For every alpha of ``alphas``
    in turn (``None``: ``ALPHA_DEFAULTS``), BP4 with message strength alpha runs up to ``num_iter`` iterations with its check outputs
    multiplied by ``factor / alpha``, from zero messages or, with ``restart=False``, from the messages the alpha before left; the first
    estimate that reproduces both syndromes is the result.  One alpha is MBP4; ``alphas=(1.0,)`` is flooding BP4 that stops at its
    first solution.

    Call ``decoder((llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs]))`` as ``QLDPCBPDecoder``: the result is
    ``(x_hat, z_hat)`` [bs,n] in its dtypes (int64 and float64).  ``last_stats[bs,4]`` (int32) = solution found, the index of the alpha
    of the last test, iterations run, and the iteration within that alpha of the last test; ``last_alpha[bs]`` (float32) = the alpha
    that solved the sample, NaN where none did."""

    def __init__(self, code, alphas=None, num_iter=64, cn_type="minsum", factor=0.8, restart=True, device=None, graph=None):
        alphas = ALPHA_DEFAULTS if alphas is None else tuple(float(x) for x in alphas)
        if not 1 <= len(alphas) <= MAX_ALPHAS:
            raise ValueError(f"alphas must hold 1 .. {MAX_ALPHAS} values")
        if not all(np.isfinite(x) and x > 0 for x in alphas):
            raise ValueError("every alpha must be finite and positive")
        if not isinstance(num_iter, (int, np.integer)) or num_iter < 1:
            raise ValueError("num_iter must be a positive integer")
        if not (np.isfinite(float(factor)) and float(factor) > 0):
            raise ValueError("factor must be finite and positive")
        if cn_type not in CN_TYPES:
            raise ValueError("Unknown node type.")
        self._code = code
        self.alphas, self.num_iter, self.cn_type, self.factor, self.restart = alphas, int(num_iter), cn_type, float(factor), bool(restart)
        self.factors, self.owns = mbp4_tables(alphas, factor)
        if not np.isfinite(self.factors).all():
            raise ValueError("factor / alpha must be finite in float32")
        if graph is None:
            from .graph import TannerGraph
            graph = TannerGraph(code, stage_one=False, device=device)
        self.graph = graph
        self._num_vns, self._num_cns_x, self._num_cns_z = self.graph.n, self.graph.m_x, self.graph.m_z
        self.last_stats = self.last_alpha = None

    code = property(lambda self: self._code)
    num_vns = property(lambda self: self._num_vns)

    def solving_alpha(self, stats):
        """[B] float32: the alpha of the attempt in which the sample was solved (``stats[:, 1]``), NaN for an unsolved sample."""
        table = torch.from_numpy(self.owns).to(stats.device)
        alpha = table[stats[:, 1].long()]
        return torch.where(stats[:, 0] > 0, alpha, torch.full_like(alpha, float("nan")))

    def decode(self, synd_x, synd_z, llr_ch=None, llr_const=0.0, first_sample=0, seed=None):
        """Estimates and stats for syndromes [B, m_x] / [B, m_z] (uint8, device) under ``llr_ch`` [B, 3, n] or one LLR for everything.
        ``first_sample`` and ``seed`` are taken and ignored, so that the decoder can stand where a ``BP4FeedbackDecoder`` does: AMBP4
        draws nothing."""
        x_hat, z_hat, stats = self.graph.mbp4_decode(synd_x, synd_z, self.factors, self.owns, self.num_iter, self.num_iter, self.cn_type,
                                                     restart=self.restart, llr_ch=llr_ch, llr_const=llr_const)
        self.last_stats, self.last_alpha = stats, self.solving_alpha(stats)
        return x_hat, z_hat, stats

    def __call__(self, inputs):
        g = self.graph
        llr_ch, syndrome_x, syndrome_z = inputs
        llr_ch = torch.as_tensor(llr_ch, device=g.device)
        if llr_ch.dtype != torch.float32:
            raise TypeError('Invalid input dtype.')
        if llr_ch.shape[-1] != self._num_vns:
            raise ValueError('Last dimension must be of length n.')
        if llr_ch.dim() != 3 or llr_ch.shape[1] != 3:
            raise ValueError('llr_ch must have shape [batch_size, 3, n].')
        synd = []
        for s, rows in ((syndrome_x, self._num_cns_x), (syndrome_z, self._num_cns_z)):
            s = torch.as_tensor(s, device=g.device)
            if s.dim() != 2 or s.shape[0] != rows:
                raise ValueError(f"syndrome must have shape [{rows}, batch_size], got {tuple(s.shape)}")
            if s.shape[1] != llr_ch.shape[0]:
                raise ValueError('batch sizes of llr_ch and the syndromes differ.')
            synd.append((s.to(torch.int64) & 1).to(torch.uint8).t().contiguous())
        x_hat, z_hat, _ = self.decode(synd[0], synd[1], llr_ch=llr_ch.contiguous())
        return x_hat.to(torch.int64), z_hat.to(torch.float64)

    call = __call__


class BP4_AMBP_Model:
    """``BP4_AMBP_Model(code, decoder, p0=None)``; ``model(batch_size, p)`` → ``(s_hat[bs, m_z+m_x], ls_hat[bs,
    rows(hx_perp)+rows(hz_perp)])``, shaped like ``BP4_Feedback_Model``: depolarizing noise of rate ``p`` from the stream of ``seed``,
    its two syndromes, AMBP4 under the prior ``log(3(1-p0)/p0)`` (``p0=None``: of ``p`` itself).  ``s_hat`` is non-zero exactly on the
    samples for which no solution was found.  After a call ``last_noise_x``, ``last_noise_z``, ``last_x_hat``, ``last_z_hat`` (uint8
    [bs,n]), ``last_stats`` (int32 [bs,4]), ``last_alpha`` (float32 [bs]) and ``last_num_unsolved`` describe that batch.  ``rank`` /
    ``world_size`` shard the sample stream by global sample index: a shard decodes its samples exactly as a single process would."""

    def __init__(self, code, decoder, p0=None, *, seed=0x5EED, rank=0, world_size=1):
        self.code, self.decoder, self.p0 = code, decoder, p0
        self.graph = decoder.graph
        self.seed, self.rank, self.world_size, self._next = int(seed), int(rank), int(world_size), 0
        self.last_noise_x = self.last_noise_z = self.last_x_hat = self.last_z_hat = self.last_stats = self.last_alpha = None
        self.last_num_unsolved = 0

    def next_sample_range(self, batch_size):
        """``(first, last)``: the half-open range of global sample indices this rank's next batch will draw."""
        first = self._next + self.rank * int(batch_size)
        return first, first + int(batch_size)

    def __call__(self, batch_size, ebno_db=None, **kw):
        p = float(kw.get("p", ebno_db))
        B, g, d = int(batch_size), self.graph, self.decoder
        first = self._next + self.rank * B
        self._next += self.world_size * B
        p0 = np.float32(p if self.p0 is None else self.p0)
        llr_const = float(np.log(np.float32(3.0) * (np.float32(1.0) - p0) / p0, dtype=np.float32))
        ex, ez = g.pauli_noise(self.seed, p, first, B)
        sx, sz = g.syndrome(ex, ez)
        x_hat, z_hat, stats = d.decode(sx, sz, llr_const=llr_const)
        self.last_noise_x, self.last_noise_z, self.last_x_hat, self.last_z_hat, self.last_stats = ex, ez, x_hat, z_hat, stats
        self.last_alpha = d.last_alpha
        self.last_num_unsolved = int((stats[:, 0] == 0).sum().item())
        s_hat, ls_hat, _ = g.residual(ex, ez, x_hat, z_hat, want_arrays=True)
        return s_hat, ls_hat

    call = __call__
