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

from ._frontend import CodeDecoder, DepolarizingBP4Model, alpha_list, bsc_logit, llr_ch_in, syndrome_in
from .mbp import MAX_ALPHAS, mbp4_tables


class SoftSyndromeBP4Decoder(CodeDecoder):
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
        alphas = alpha_list(alphas, MAX_ALPHAS, num_iter, factor, cn_type)
        self.alphas, self.num_iter, self.cn_type, self.factor, self.restart = alphas, int(num_iter), cn_type, float(factor), bool(restart)
        self.factors, self.owns = mbp4_tables(alphas, factor)
        if not np.isfinite(self.factors).all():
            raise ValueError("factor / alpha must be finite in float32")
        self._attach(code, graph, device)
        self.last_u_x_hat = self.last_u_z_hat = None

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
        device = self.graph.device
        llr_ch, syndrome_x, syndrome_z, synd_llr_x, synd_llr_z = inputs
        llr_ch = llr_ch_in(llr_ch, self._num_vns, device)
        synd, soft = [], []
        for s, lr, rows in ((syndrome_x, synd_llr_x, self._num_cns_x), (syndrome_z, synd_llr_z, self._num_cns_z)):
            synd.append(syndrome_in(s, rows, device, llr_ch.shape[0]))
            if lr is not None:
                lr = torch.as_tensor(lr, device=device)
                if tuple(lr.shape) != (rows, llr_ch.shape[0]):
                    raise ValueError(f"syndrome LLRs must have shape {(rows, llr_ch.shape[0])}, got {tuple(lr.shape)}")
                lr = lr.to(torch.float32).t().contiguous()
            soft.append(lr)
        x_hat, z_hat = self.decode(synd[0], synd[1], soft[0], soft[1], llr_ch=llr_ch)[:2]
        return x_hat.to(torch.int64), z_hat.to(torch.float64)

    call = __call__


class BP4_SoftSyndrome_Model(DepolarizingBP4Model):
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
        super().__init__(code, decoder, p0, seed=seed, rank=rank, world_size=world_size)
        self.q, self.q0 = q, q0
        self.last_u_x = self.last_u_z = self.last_u_x_hat = self.last_u_z_hat = None

    @property
    def gamma(self):
        """``log((1-q0)/q0)`` in float32 arithmetic, +inf for ``q0 = 0``."""
        q0 = self.q if self.q0 is None else self.q0
        return float("inf") if np.float32(q0) == 0 else -bsc_logit(q0)

    def _measure(self, sx, sz, first, B):
        if self.q > 0:
            ux, uz = self.graph.syndrome_noise(self.seed, self.q, first, B)
            sx, sz = sx ^ ux, sz ^ uz
        else:
            ux, uz = torch.zeros_like(sx), torch.zeros_like(sz)
        self.last_u_x, self.last_u_z = ux, uz
        return sx, sz

    def _decode(self, sx, sz, llr_const, first):
        x_hat, z_hat, self.last_u_x_hat, self.last_u_z_hat, stats = self.decoder.decode(sx, sz, gamma=self.gamma, llr_const=llr_const)
        return x_hat, z_hat, stats
