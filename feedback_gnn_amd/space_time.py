"""Space-time BP4 on MI355X: repeated noisy syndrome measurements decoded together (the phenomenological noise model of
fault-tolerant memory experiments), flooding schedule.

`SoftSyndromeBP4Decoder` decodes one round of measurement, and one round cannot tell a flipped syndrome bit from a data error next to
it.  Here a window of ``rounds`` consecutive measurements is one decoding problem: the differences of consecutive syndromes are R
copies of the code's two Tanner graphs, coupled by one binary "time" variable per check and round (the flip of that measured bit),
and the decoder estimates the data error of every round next to the flips.  The algorithm is stated at `fgnn_stbp4_decode` in
include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_stbp4.hip: one launch, the messages of the whole window in LDS throughout, and
AMBP4's alpha list kept.  Experiments longer than a window are decoded as sliding windows (`BP4_Phenomenological_Model`).
"""
import numpy as np
import torch

from ._frontend import CodeDecoder, ShardedModel, alpha_list, bsc_logit, depolarizing_llr, llr_ch_in
from .mbp import MAX_ALPHAS, mbp4_tables

INF = float("inf")


def _xor_rounds(t):
    """XOR over dimension 1 of a uint8 [B, R, k] tensor."""
    return (t.sum(dim=1, dtype=torch.int32) & 1).to(torch.uint8)


class SpaceTimeBP4Decoder(CodeDecoder):
    """``SpaceTimeBP4Decoder(code, rounds, alphas=(1.0,), num_iter=64, cn_type="minsum", factor=0.8, restart=True)``: windows of up
    to ``rounds`` measurements; ``alphas``, ``num_iter``, ``cn_type``, ``factor`` and ``restart`` as `SoftSyndromeBP4Decoder`.

    ``decode(synd_x[B,R,m_x], synd_z[B,R,m_z], prev_x=None, prev_z=None, synd_llr_x=None, synd_llr_z=None, gamma=inf, gamma_last=inf,
    ...)`` returns ``(x_hat[B,R,n], z_hat[B,R,n], u_x_hat[B,R,m_x], u_z_hat[B,R,m_z], stats[B,4])``: the error estimated for each round
    (not cumulative), the measured bits estimated wrong, and per window solution found, the index of the alpha of the last test,
    iterations run, and the iteration within that alpha of the last test.  R may be anything from 1 to ``rounds``.  After a call
    ``last_correction_x`` / ``last_correction_z`` [B,n] (uint8) are the XOR of the per-round estimates, ``last_u_x_hat`` /
    ``last_u_z_hat`` and ``last_stats`` the other outputs.

    Call ``decoder((llr_ch[bs,3,n], syndrome_x[R,m_x,bs], syndrome_z[R,m_z,bs]))`` with the rounds of a window stacked in front of the
    syndrome layout of ``QLDPCBPDecoder``: the result is the total correction ``(x_hat, z_hat)`` [bs,n] in its dtypes (int64 and
    float64), decoded under the attributes ``gamma`` and ``gamma_last`` (both +inf unless set)."""

    def __init__(self, code, rounds, alphas=(1.0,), num_iter=64, cn_type="minsum", factor=0.8, restart=True, device=None, graph=None):
        if not isinstance(rounds, (int, np.integer)) or rounds < 1:
            raise ValueError("rounds must be a positive integer")
        alphas = alpha_list(alphas, MAX_ALPHAS, num_iter, factor, cn_type)
        self.rounds = int(rounds)
        self.alphas, self.num_iter, self.cn_type, self.factor, self.restart = alphas, int(num_iter), cn_type, float(factor), bool(restart)
        self.factors, self.owns = mbp4_tables(alphas, factor)
        if not np.isfinite(self.factors).all():
            raise ValueError("factor / alpha must be finite in float32")
        self._attach(code, graph, device)
        self.gamma = self.gamma_last = INF
        self.last_u_x_hat = self.last_u_z_hat = self.last_correction_x = self.last_correction_z = None

    def decode(self, synd_x, synd_z, prev_x=None, prev_z=None, synd_llr_x=None, synd_llr_z=None, gamma=INF, gamma_last=INF, llr_ch=None,
               llr_const=0.0, rounds=None):
        """Estimates and stats for the raw syndromes [B, R, m_x] / [B, R, m_z] (uint8, device) of a window that starts from the
        syndrome ``prev_x`` / ``prev_z`` [B, m] (None: zero), under syndrome LLRs [B, R, m] (float32) or ``gamma`` for rounds 0 .. R-2
        and ``gamma_last`` for round R-1 of a side whose array is None, and ``llr_ch`` [B, 3, n] or one LLR for everything."""
        given = next((t for t in (synd_x, synd_z, synd_llr_x, synd_llr_z) if t is not None), None)
        R = int(rounds) if rounds is not None else (int(given.shape[1]) if given is not None and given.dim() == 3 else self.rounds)
        if R > self.rounds:
            raise ValueError(f"a window holds at most {self.rounds} rounds, got {R}")
        x_hat, z_hat, u_x_hat, u_z_hat, stats = self.graph.stbp4_decode(
            synd_x, synd_z, self.factors, self.owns, self.num_iter, self.num_iter, self.cn_type, restart=self.restart, rounds=R,
            prev_x=prev_x, prev_z=prev_z, llr_ch=llr_ch, llr_const=llr_const, synd_llr_x=synd_llr_x, synd_llr_z=synd_llr_z,
            gamma_x=gamma, gamma_z=gamma, gamma_last_x=gamma_last, gamma_last_z=gamma_last)
        self.last_stats, self.last_u_x_hat, self.last_u_z_hat = stats, u_x_hat, u_z_hat
        self.last_correction_x, self.last_correction_z = _xor_rounds(x_hat), _xor_rounds(z_hat)
        return x_hat, z_hat, u_x_hat, u_z_hat, stats

    def __call__(self, inputs):
        device = self.graph.device
        llr_ch, syndrome_x, syndrome_z = inputs
        llr_ch = llr_ch_in(llr_ch, self._num_vns, device)
        bs = llr_ch.shape[0]
        synd = []
        for s, rows in ((syndrome_x, self._num_cns_x), (syndrome_z, self._num_cns_z)):
            s = torch.as_tensor(s, device=device)
            if s.dim() != 3 or s.shape[1] != rows:
                raise ValueError(f"syndrome must have shape [rounds, {rows}, batch_size], got {tuple(s.shape)}")
            if s.shape[2] != bs:
                raise ValueError('batch sizes of llr_ch and the syndromes differ.')
            synd.append((s.to(torch.int64) & 1).to(torch.uint8).permute(2, 0, 1).contiguous())
        if synd[0].shape[1] != synd[1].shape[1]:
            raise ValueError("the two syndromes must hold the same number of rounds")
        self.decode(synd[0], synd[1], gamma=self.gamma, gamma_last=self.gamma_last, llr_ch=llr_ch)
        return self.last_correction_x.to(torch.int64), self.last_correction_z.to(torch.float64)

    call = __call__


class BP4_Phenomenological_Model(ShardedModel):
    """``BP4_Phenomenological_Model(code, decoder, q, rounds, window=None, commit=None, p0=None, q0=None, seed=..)``; ``model(batch_size,
    p)`` → ``(s_hat[bs, m_z+m_x], ls_hat[bs, rows(hx_perp)+rows(hz_perp)])``, shaped like ``BP4_SoftSyndrome_Model``.  A sample is a
    memory experiment of ``rounds`` measurements: before each one a fresh depolarizing error of rate ``p`` joins the accumulated
    error; measurements 0 .. rounds-2 report its two syndromes with flips of rate ``q``, the last one reports them exactly.  The draws
    are rows ``first * rounds .. (first + bs) * rounds - 1`` of `TannerGraph.pauli_noise` / `TannerGraph.syndrome_noise` on ``seed``,
    viewed as ``[bs, rounds, .]``, so a shard (``rank`` / ``world_size``) decodes its samples as a single process would.  The decoder
    is a `SpaceTimeBP4Decoder`; the prior is ``log(3(1-p0)/p0)`` (``p0=None``: of ``p``), the syndrome LLR ``gamma = log((1-q0)/q0)``
    (``q0=None``: of ``q``; +inf for 0).

    With ``window=None`` or ``rounds <= window`` one launch decodes all rounds with ``gamma_last = +inf``.  Otherwise windows of
    ``window`` rounds start at rounds 0, F, 2F, .. with F = ``commit`` (1 <= F <= window; ``commit=None`` means F = 1, the most overlap).  A window that does not reach the final round decodes with ``gamma_last = gamma``,
    commits the estimates of its first F rounds and hands ``prev = s_{a+F-1} ^ u_hat_{a+F-1}`` to the next; the first window that
    reaches the final round is the last: it decodes what is left with ``gamma_last = +inf`` and commits all its rounds.

    ``s_hat`` and ``ls_hat`` are those of the residual: the XOR of all drawn errors ^ the XOR of all committed estimates.  After a
    call ``last_noise_x``, ``last_noise_z``, ``last_x_hat``, ``last_z_hat`` (uint8 [bs,rounds,n]: drawn and committed per round),
    ``last_u_x``, ``last_u_z``, ``last_u_x_hat``, ``last_u_z_hat`` (uint8 [bs,rounds,m]), ``last_stats`` (int32 [bs,4], of the last
    window), ``last_window_stats`` (one per window) and ``last_num_unsolved`` (the number of windows not solved, over the batch)
    describe that batch."""

    def __init__(self, code, decoder, q, rounds, window=None, commit=None, p0=None, q0=None, *, seed=0x5EED, rank=0, world_size=1):
        q = float(q)
        if not 0.0 <= q < 1.0:
            raise ValueError("q must be in [0, 1)")
        if q0 is not None and not 0.0 <= float(q0) < 1.0:
            raise ValueError("q0 must be in [0, 1)")
        if not isinstance(rounds, (int, np.integer)) or rounds < 1:
            raise ValueError("rounds must be a positive integer")
        if window is not None:
            if not isinstance(window, (int, np.integer)) or window < 1:
                raise ValueError("window must be a positive integer")
            commit = 1 if commit is None else commit
            if not isinstance(commit, (int, np.integer)) or not 1 <= commit <= window:
                raise ValueError("commit must be in 1 .. window")
        elif commit is not None:
            raise ValueError("commit needs a window")
        if min(int(rounds), int(window) if window is not None else int(rounds)) > decoder.rounds:
            raise ValueError(f"the decoder's windows hold at most {decoder.rounds} rounds")
        self.code, self.decoder, self.p0, self.q, self.q0 = code, decoder, p0, q, q0
        self.rounds, self.window, self.commit = int(rounds), None if window is None else int(window), None if commit is None else int(commit)
        self.graph = decoder.graph
        self._shard(seed, rank, world_size)
        self.last_noise_x = self.last_noise_z = self.last_x_hat = self.last_z_hat = self.last_stats = None
        self.last_u_x = self.last_u_z = self.last_u_x_hat = self.last_u_z_hat = self.last_window_stats = None
        self.last_num_unsolved = 0

    @property
    def gamma(self):
        """``log((1-q0)/q0)`` in float32 arithmetic, +inf for ``q0 = 0``."""
        q0 = self.q if self.q0 is None else self.q0
        return INF if np.float32(q0) == 0 else -bsc_logit(q0)

    def windows(self):
        """``[(first round, rounds in the window, rounds committed, is the last)]``."""
        R, W, F = self.rounds, self.window, self.commit
        if W is None or R <= W:
            return [(0, R, R, True)]
        plan, a = [], 0
        while a + W < R:
            plan.append((a, W, F, False))
            a += F
        plan.append((a, R - a, R - a, True))
        return plan

    def __call__(self, batch_size, ebno_db=None, **kw):
        p = float(kw.get("p", ebno_db))
        B, g, R = int(batch_size), self.graph, self.rounds
        first = self._take(B)
        llr_const = depolarizing_llr(p if self.p0 is None else self.p0)
        ex, ez = g.pauli_noise(self.seed, p, first * R, B * R)
        ex, ez = ex.view(B, R, g.n), ez.view(B, R, g.n)
        cx, cz = ex.clone(), ez.clone()  # the accumulated error at each measurement
        for t in range(1, R):
            cx[:, t] ^= cx[:, t - 1]
            cz[:, t] ^= cz[:, t - 1]
        sx, sz = g.syndrome(cx.view(B * R, g.n), cz.view(B * R, g.n))
        sx, sz = sx.view(B, R, g.m_x), sz.view(B, R, g.m_z)
        if self.q > 0:
            ux, uz = g.syndrome_noise(self.seed, self.q, first * R, B * R)
            ux, uz = ux.view(B, R, g.m_x), uz.view(B, R, g.m_z)
            ux[:, R - 1] = 0  # the last measurement is perfect: its draws are made and dropped
            uz[:, R - 1] = 0
            sx, sz = sx ^ ux, sz ^ uz
        else:
            ux, uz = torch.zeros_like(sx), torch.zeros_like(sz)
        gamma = self.gamma
        out = [torch.zeros_like(t) for t in (ex, ez, ux, uz)]
        stats_all, unsolved, px, pz = [], 0, None, None
        for a, W, F, last in self.windows():
            xh, zh, uxh, uzh, stats = self.decoder.decode(sx[:, a:a + W].contiguous(), sz[:, a:a + W].contiguous(), prev_x=px, prev_z=pz,
                                                          gamma=gamma, gamma_last=INF if last else gamma, llr_const=llr_const)
            for o, t in zip(out, (xh, zh, uxh, uzh)):
                o[:, a:a + F] = t[:, :F]
            stats_all.append(stats)
            unsolved += int((stats[:, 0] == 0).sum().item())
            if not last:
                px, pz = (sx[:, a + F - 1] ^ uxh[:, F - 1]).contiguous(), (sz[:, a + F - 1] ^ uzh[:, F - 1]).contiguous()
        self.last_noise_x, self.last_noise_z, self.last_u_x, self.last_u_z = ex, ez, ux, uz
        self.last_x_hat, self.last_z_hat, self.last_u_x_hat, self.last_u_z_hat = out
        self.last_stats, self.last_window_stats, self.last_num_unsolved = stats_all[-1], stats_all, unsolved
        s_hat, ls_hat, _ = g.residual(cx[:, R - 1].contiguous(), cz[:, R - 1].contiguous(), _xor_rounds(out[0]), _xor_rounds(out[1]),
                                      want_arrays=True)
        return s_hat, ls_hat

    call = __call__
