"""Soft-syndrome BP4 on MI355X: data and syndrome errors decoded together (Kuo, Chern, Lai, "Decoding of quantum data-syndrome codes
via belief propagation", 2021; Raveendran et al., "Soft syndrome decoding of quantum LDPC codes for joint correction of data and
syndrome errors", 2022; Berent et al., "Analog information decoding of bosonic quantum LDPC codes", 2023), flooding schedule.

Every other decoder of the package takes the measured syndrome as exact.  Here check ``c`` carries a log-likelihood ratio ``gamma_c``
that says how far its measured bit can be trusted; the check rule takes it as one more input, the decoder estimates which syndrome
bits were wrong (``u_hat``) next to the data error, and a sample is solved when ``H e_hat == s ^ u_hat`` on both graphs.  The
algorithm is stated at `fgnn_dsbp4_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_dsbp4.hip: one launch, the
messages, decisions and ``u_hat`` bytes of a codeword in LDS throughout, and AMBP4's alpha list kept.
"""
import numpy as np
import torch

from ._lib import CN_TYPES
from .mbp import MAX_ALPHAS, mbp4_tables


class SoftSyndromeBP4Decoder:
    """``SoftSyndromeBP4Decoder(code, alphas=(1.0,), num_iter=64, cn_type="minsum", factor=0.8, restart=True)``.  One alpha of 1.0 is
    plain soft-syndrome flooding BP4; a descending list is Kuo, Chern and Lai's MBP4 on the data-syndrome code: for every alpha in turn
    up to ``num_iter`` iterations with the check outputs multiplied by ``factor / alpha``, from zero messages or, with
    ``restart=False``, from the messages the alpha before left.

    ``decode(synd_x, synd_z, synd_llr_x=None, synd_llr_z=None, gamma=inf, ...)`` returns ``(x_hat, z_hat, u_x_hat, u_z_hat, stats)``.
    Call ``decoder((llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs], synd_llr_x[m_x,bs], synd_llr_z[m_z,bs]))`` in the
    syndrome layout of ``QLDPCBPDecoder``: the result is ``(x_hat, z_hat)`` [bs,n] in its dtypes (int64 and float64).  After either,
    ``last_stats[bs,4]`` (int32) = solution found, the index of the alpha of the last test, iterations run, and the iteration within
    that alpha of the last test; ``last_u_x_hat[bs,m_x]`` and ``last_u_z_hat[bs,m_z]`` (uint8) = the syndrome bits estimated wrong."""

    def __init__(self, code, alphas=(1.0,), num_iter=64, cn_type="minsum", factor=0.8, restart=True, device=None, graph=None):
        alphas = tuple(float(x) for x in alphas)
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
        self.last_stats = self.last_u_x_hat = self.last_u_z_hat = None

    code = property(lambda self: self._code)
    num_vns = property(lambda self: self._num_vns)

    @staticmethod
    def from_soft(values):
        """Signed analog syndromes to ``(bits, llr)``: the bit is 1 where the value is negative, the LLR is the magnitude.  Same shape;
        uint8 and float32."""
        values = torch.as_tensor(values)
        return (values < 0).to(torch.uint8), values.abs().to(torch.float32)

    def decode(self, synd_x, synd_z, synd_llr_x=None, synd_llr_z=None, gamma=float("inf"), llr_ch=None, llr_const=0.0):
        """Estimates and stats for syndromes [B, m_x] / [B, m_z] (uint8, device) under syndrome LLRs [B, m_x] / [B, m_z] (float32), or
        ``gamma`` for every check of a side whose array is None, and ``llr_ch`` [B, 3, n] or one LLR for everything."""
        x_hat, z_hat, u_x_hat, u_z_hat, stats = self.graph.dsbp4_decode(
            synd_x, synd_z, self.factors, self.owns, self.num_iter, self.num_iter, self.cn_type, restart=self.restart, llr_ch=llr_ch,
            llr_const=llr_const, synd_llr_x=synd_llr_x, synd_llr_z=synd_llr_z, gamma_x=gamma, gamma_z=gamma)
        self.last_stats, self.last_u_x_hat, self.last_u_z_hat = stats, u_x_hat, u_z_hat
        return x_hat, z_hat, u_x_hat, u_z_hat, stats

    def __call__(self, inputs):
        g = self.graph
        llr_ch, syndrome_x, syndrome_z, synd_llr_x, synd_llr_z = inputs
        llr_ch = torch.as_tensor(llr_ch, device=g.device)
        if llr_ch.dtype != torch.float32:
            raise TypeError('Invalid input dtype.')
        if llr_ch.shape[-1] != self._num_vns:
            raise ValueError('Last dimension must be of length n.')
        if llr_ch.dim() != 3 or llr_ch.shape[1] != 3:
            raise ValueError('llr_ch must have shape [batch_size, 3, n].')
        synd, soft = [], []
        for s, lr, rows in ((syndrome_x, synd_llr_x, self._num_cns_x), (syndrome_z, synd_llr_z, self._num_cns_z)):
            s = torch.as_tensor(s, device=g.device)
            if s.dim() != 2 or s.shape[0] != rows:
                raise ValueError(f"syndrome must have shape [{rows}, batch_size], got {tuple(s.shape)}")
            if s.shape[1] != llr_ch.shape[0]:
                raise ValueError('batch sizes of llr_ch and the syndromes differ.')
            synd.append((s.to(torch.int64) & 1).to(torch.uint8).t().contiguous())
            if lr is not None:
                lr = torch.as_tensor(lr, device=g.device)
                if tuple(lr.shape) != tuple(s.shape):
                    raise ValueError(f"syndrome LLRs must have shape {tuple(s.shape)}, got {tuple(lr.shape)}")
                lr = lr.to(torch.float32).t().contiguous()
            soft.append(lr)
        x_hat, z_hat, _, _, _ = self.decode(synd[0], synd[1], soft[0], soft[1], llr_ch=llr_ch.contiguous())
        return x_hat.to(torch.int64), z_hat.to(torch.float64)

    call = __call__


class BP4_SoftSyndrome_Model:
    """``BP4_SoftSyndrome_Model(code, decoder, q, p0=None, q0=None, seed=..)``; ``model(batch_size, p)`` → ``(s_hat[bs, m_z+m_x],
    ls_hat[bs, rows(hx_perp)+rows(hz_perp)])``, shaped like ``BP4_AMBP_Model``: depolarizing noise of rate ``p`` from the stream of
    ``seed``, its two syndromes ``s``, measurement flips ``u`` of rate ``q`` (`TannerGraph.syndrome_noise` on the same ``seed``), and
    soft-syndrome BP4 of ``s ^ u`` under the prior ``log(3(1-p0)/p0)`` (``p0=None``: of ``p`` itself) and the syndrome LLR ``gamma =
    log((1-q0)/q0)`` (``q0=None``: of ``q``).  ``q = 0`` draws no flips and gives ``gamma = +inf``.

    Unlike the sibling models, ``s_hat`` can be non-zero on a solved sample: the stop test is ``H e_hat == (s ^ u) ^ u_hat``, so the
    residual syndrome ``H (e ^ e_hat) = u ^ u_hat`` is non-zero exactly where ``u_hat != u``.  After a call ``last_noise_x``,
    ``last_noise_z``, ``last_x_hat``, ``last_z_hat`` (uint8 [bs,n]), ``last_u_x``, ``last_u_z``, ``last_u_x_hat``, ``last_u_z_hat``
    (uint8 [bs,m_x] / [bs,m_z]), ``last_stats`` (int32 [bs,4]) and ``last_num_unsolved`` describe that batch.  ``rank`` /
    ``world_size`` shard the sample streams by global sample index: a shard decodes its samples exactly as a single process would."""

    def __init__(self, code, decoder, q, p0=None, q0=None, *, seed=0x5EED, rank=0, world_size=1):
        q = float(q)
        if not 0.0 <= q < 1.0:
            raise ValueError("q must be in [0, 1)")
        if q0 is not None and not 0.0 <= float(q0) < 1.0:
            raise ValueError("q0 must be in [0, 1)")
        self.code, self.decoder, self.q, self.p0, self.q0 = code, decoder, q, p0, q0
        self.graph = decoder.graph
        self.seed, self.rank, self.world_size, self._next = int(seed), int(rank), int(world_size), 0
        self.last_noise_x = self.last_noise_z = self.last_x_hat = self.last_z_hat = self.last_stats = None
        self.last_u_x = self.last_u_z = self.last_u_x_hat = self.last_u_z_hat = None
        self.last_num_unsolved = 0

    @property
    def gamma(self):
        """``log((1-q0)/q0)`` in float32 arithmetic, +inf for ``q0 = 0``."""
        q0 = np.float32(self.q if self.q0 is None else self.q0)
        if q0 == 0:
            return float("inf")
        return float(np.log((np.float32(1.0) - q0) / q0, dtype=np.float32))

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
        if self.q > 0:
            ux, uz = g.syndrome_noise(self.seed, self.q, first, B)
            sx, sz = sx ^ ux, sz ^ uz
        else:
            ux, uz = torch.zeros_like(sx), torch.zeros_like(sz)
        x_hat, z_hat, u_x_hat, u_z_hat, stats = d.decode(sx, sz, gamma=self.gamma, llr_const=llr_const)
        self.last_noise_x, self.last_noise_z, self.last_x_hat, self.last_z_hat, self.last_stats = ex, ez, x_hat, z_hat, stats
        self.last_u_x, self.last_u_z, self.last_u_x_hat, self.last_u_z_hat = ux, uz, u_x_hat, u_z_hat
        self.last_num_unsolved = int((stats[:, 0] == 0).sum().item())
        s_hat, ls_hat, _ = g.residual(ex, ez, x_hat, z_hat, want_arrays=True)
        return s_hat, ls_hat

    call = __call__
