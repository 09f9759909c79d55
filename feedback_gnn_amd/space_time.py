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

    def _window_in(self, inputs):
        """``(synd_x [bs,R,m_x], synd_z [bs,R,m_z], llr_ch [bs,3,n])`` of a ``(llr_ch, syndrome_x, syndrome_z)`` call."""
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
        return synd[0], synd[1], llr_ch

    def __call__(self, inputs):
        synd_x, synd_z, llr_ch = self._window_in(inputs)
        self.decode(synd_x, synd_z, gamma=self.gamma, gamma_last=self.gamma_last, llr_ch=llr_ch)
        return self.last_correction_x.to(torch.int64), self.last_correction_z.to(torch.float64)

    call = __call__


def window_matrix(h, rounds):
    """One side of a window of ``rounds`` measurements as the binary matrix ``H_st`` (uint8, host) of ``H_st [e ; u] = d``: check
    (c,t) is row ``t m + c``, data bit (v,t) column ``t n + v`` and time bit (c,t) column ``R n + t m + c``, with ``h [m,n]`` on the
    block diagonal and ones at time bits (c,t) and (c,t-1) of row (c,t).  The time columns are unit lower-bidiagonal, so the rank is
    ``R m``; ``rounds = 1`` gives ``[h | I]``.  The layout is that of `fgnn_st_window_problem` (include/fgnn.h)."""
    h = (np.asarray(h) != 0).astype(np.uint8)
    if not isinstance(rounds, (int, np.integer)) or rounds < 1:
        raise ValueError("rounds must be a positive integer")
    R, (m, n) = int(rounds), h.shape
    H = np.zeros((R * m, R * (n + m)), np.uint8)
    eye = np.arange(m)
    for t in range(R):
        H[t * m:(t + 1) * m, t * n:(t + 1) * n] = h
        H[t * m + eye, R * n + t * m + eye] = 1
        if t > 0:
            H[t * m + eye, R * n + (t - 1) * m + eye] = 1
    return H


LSD_MAX_CHECKS = 8192   # fgnn_lsd: checks per side
OSD_MAX_BITS = 16384    # fgnn_osd_ws: columns
POST_METHODS = ("lsd", "osd0")


class SpaceTimePostDecoder:
    """``SpaceTimePostDecoder(decoder, method="lsd", max_pivots=None, max_rounds=None, fallback="osd0")``: a `SpaceTimeBP4Decoder`
    with a post-processor behind it.  ``decode(...)`` takes the arguments of `SpaceTimeBP4Decoder.decode` and returns the same five
    outputs; ``rounds``, ``graph``, the call with ``(llr_ch, syndrome_x, syndrome_z)`` and the ``last_*`` attributes are the
    decoder's too, so `BP4_Phenomenological_Model` takes it in the decoder's place, sliding windows included.

    The window is decoded by `TannerGraph.stbp4_decode_soft`.  The windows it leaves unsolved are compacted, and each of their two
    sides is solved as the binary problem ``H_st [e ; u] = d`` (`window_matrix`, `TannerGraph.st_window_problem`) on the binary
    LLRs of the qubits' last marginals and the Gamma of the time variables: by LSD (``method="lsd"``: `fgnn_lsd` with ``max_pivots``
    / ``max_rounds`` as `LSD_Decoder`), by OSD-0 on the basis of all rows (``method="osd0"``), or by LSD and then OSD-0 for the
    windows LSD returns with found = 0 on either side (``fallback="osd0"``; ``fallback=None`` leaves them as LSD's read-out), as
    `BP4_LSD_Model`.  The solutions replace the estimates of those windows (`TannerGraph.st_window_apply`) and ``stats[:,0]``
    becomes 1 where both sides came back found: the estimate then satisfies the window's checks, and with them the hand-over ``s ^
    u_hat`` to the next window does.  Solved windows are returned exactly as `SpaceTimeBP4Decoder` returns them.

    After a call ``last_num_post`` counts the windows post-processed, ``last_num_fallback`` those handed on to OSD-0, and
    ``last_post_stats`` [2, B, 4] int32 holds `fgnn_lsd`'s stats (found, rounds, columns, pivots) of side 0 (hx) and 1 (hz), the
    rows of untouched windows (and every row under ``method="osd0"``) reading "found, nothing done".  A window whose side has more
    than 8192 checks is beyond `fgnn_lsd`, one with more than 16384 columns beyond OSD-0: both are refused with a ValueError."""

    def __init__(self, decoder, method="lsd", max_pivots=None, max_rounds=None, fallback="osd0"):
        if method not in POST_METHODS:
            raise ValueError(f"method must be one of {POST_METHODS}")
        if fallback not in ("osd0", None):
            raise ValueError("fallback must be 'osd0' or None")
        self.decoder, self.method, self.fallback = decoder, method, fallback
        self.max_pivots = 0 if max_pivots is None else int(max_pivots)
        self.max_rounds = 0 if max_rounds is None else int(max_rounds)
        if self.max_pivots < 0 or self.max_rounds < 0:
            raise ValueError("max_pivots and max_rounds must be >= 0")
        self.rounds, self.graph, self.code = decoder.rounds, decoder.graph, decoder.code
        self.gamma = self.gamma_last = INF
        self._graphs = {}  # (side, R) -> the binary graph of window_matrix(h_side, R)
        from .bp_osd import _OsdWorkspace
        self._ws = _OsdWorkspace()  # OSD-0 on a window graph the LDS-resident kernel refuses
        self.last_stats = self.last_u_x_hat = self.last_u_z_hat = self.last_correction_x = self.last_correction_z = None
        self.last_post_stats = None
        self.last_num_post = self.last_num_fallback = 0

    @property
    def _osd_reachable(self):
        return self.method == "osd0" or self.fallback == "osd0"

    def window_graph(self, side, rounds):
        """The binary `TannerGraph` of ``window_matrix(hx or hz, rounds)`` (cached per side and rounds), with the basis of all rows
        installed when OSD-0 can be reached."""
        key = (int(side), int(rounds))
        if key not in self._graphs:
            from .decoding import _binary_graph
            h = np.asarray(self.code.hx if side == 0 else self.code.hz)
            m, n = h.shape
            R = int(rounds)
            if self.method == "lsd" and R * m > LSD_MAX_CHECKS:
                raise ValueError(f"a window of {R} rounds has {R * m} checks on side {side}, fgnn_lsd takes at most {LSD_MAX_CHECKS}: "
                                 "use method='osd0' or a shorter window")
            if self._osd_reachable and R * (n + m) > OSD_MAX_BITS:
                raise ValueError(f"a window of {R} rounds has {R * (n + m)} columns on side {side}, OSD-0 takes at most {OSD_MAX_BITS}: "
                                 "use a shorter window" + (" or fallback=None" if self.method == "lsd" else ""))
            wg = _binary_graph(window_matrix(h, R), None, self.graph.device)
            if self._osd_reachable:
                wg.set_basis(0, np.arange(R * m, dtype=np.int32))
            self._graphs[key] = wg
        return self._graphs[key]

    def decode(self, synd_x, synd_z, prev_x=None, prev_z=None, synd_llr_x=None, synd_llr_z=None, gamma=INF, gamma_last=INF, llr_ch=None,
               llr_const=0.0, rounds=None):
        """`SpaceTimeBP4Decoder.decode` followed by the post-processing of the unsolved windows."""
        from .bp_osd import _run_osd0
        from .lsd import _fresh_stats, _missed
        d, g = self.decoder, self.graph
        given = next((t for t in (synd_x, synd_z, synd_llr_x, synd_llr_z) if t is not None), None)
        R = int(rounds) if rounds is not None else (int(given.shape[1]) if given is not None and given.dim() == 3 else self.rounds)
        if R > self.rounds:
            raise ValueError(f"a window holds at most {self.rounds} rounds, got {R}")
        x_hat, z_hat, u_x_hat, u_z_hat, stats, marg, gam_x, gam_z = g.stbp4_decode_soft(
            synd_x, synd_z, d.factors, d.owns, d.num_iter, d.num_iter, d.cn_type, restart=d.restart, rounds=R, prev_x=prev_x, prev_z=prev_z,
            llr_ch=llr_ch, llr_const=llr_const, synd_llr_x=synd_llr_x, synd_llr_z=synd_llr_z, gamma_x=gamma, gamma_z=gamma,
            gamma_last_x=gamma_last, gamma_last_z=gamma_last)
        B = int(stats.shape[0])
        index, nact = g.compact((stats[:, 0] == 0).to(torch.uint8), 1)
        self.last_num_post, self.last_num_fallback = nact, 0
        self.last_post_stats = post = _fresh_stats(g, B, 2)
        if nact:
            sides = ((synd_x, prev_x, gam_x, z_hat, u_x_hat), (synd_z, prev_z, gam_z, x_hat, u_z_hat))
            wgs = [self.window_graph(side, R) for side in (0, 1)]
            lsd_stats = _fresh_stats(g, nact, 2)  # of the compact rows
            work = []
            for side, (synd, prev, gam, _, _) in enumerate(sides):
                wg = wgs[side]
                dd, llr = g.st_window_problem(side, marg, gam, synd=synd, prev=prev, index=index, nact=nact)
                e = torch.zeros((nact, wg.n), dtype=torch.uint8, device=g.device)
                if self.method == "lsd":
                    wg.lsd(0, dd, e, llr_bin=llr, max_pivots=self.max_pivots, max_rounds=self.max_rounds, stats=lsd_stats[side])
                else:
                    _run_osd0(wg, self._ws, 0, dd, e, llr_bin=llr)
                work.append((dd, llr, e))
            found = (lsd_stats[:, :, 0] != 0).all(0)
            if self.method == "lsd" and self.fallback == "osd0":
                index2, nact2 = _missed(g, lsd_stats)
                self.last_num_fallback = nact2
                if nact2:
                    for side, (dd, llr, e) in enumerate(work):
                        _run_osd0(wgs[side], self._ws, 0, dd, e, llr_bin=llr, index=index2, nact=nact2)
                    found = torch.ones_like(found)
            for side, (_, _, _, hat, u_hat) in enumerate(sides):
                g.st_window_apply(side, work[side][2], hat, u_hat, index=index, nact=nact)
            rows = index[:nact].long()
            post[:, rows] = lsd_stats
            stats[rows, 0] = found.to(stats.dtype)
        self.last_stats, self.last_u_x_hat, self.last_u_z_hat = stats, u_x_hat, u_z_hat
        self.last_correction_x, self.last_correction_z = _xor_rounds(x_hat), _xor_rounds(z_hat)
        return x_hat, z_hat, u_x_hat, u_z_hat, stats

    def __call__(self, inputs):
        synd_x, synd_z, llr_ch = self.decoder._window_in(inputs)
        self.decode(synd_x, synd_z, gamma=self.gamma, gamma_last=self.gamma_last, llr_ch=llr_ch)
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
