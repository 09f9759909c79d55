"""BP+LSD: localized statistics decoding (LSD-0 with synchronous growth; Hillmann et al. 2024, `BpLsdDecoder` of ``ldpc`` v2) as the
post-processor of BP failures on MI355X.  The contract is stated in include/fgnn.h (`fgnn_lsd`); the models mirror `BP4_OSD_Model` and
`BP2_OSD_Model` of bp_osd.py with the cluster decoder in OSD's place.
"""
import numpy as np
import torch

from ._frontend import ShardedModel, bsc_logit, depolarizing_llr
from ._lib import ROWS_LX, ROWS_LZ
from .decoding import _bp2_stage
from .bp_osd import _OsdWorkspace, _run_osd0, _StandaloneOSD
from .feedback_gnn import Pauli

FALLBACKS = ("osd0", None)


def _fresh_stats(g, B, sides=1):
    """stats [sides, B, 4] int32 whose rows read "found, nothing done" until `lsd` overwrites the processed ones."""
    stats = torch.zeros((sides, B, 4), dtype=torch.int32, device=g.device)
    stats[:, :, 0] = 1
    return stats


def _missed(g, stats):
    """(index, count) of the samples with found = 0 in any side of stats [sides, B, 4]."""
    miss = (stats[:, :, 0] == 0).any(0).to(torch.uint8)
    return g.compact(miss, 1)


class LSD_Decoder(_StandaloneOSD):
    """``LSD_Decoder(n, max_pivots=None, max_rounds=None, fallback="osd0")``: the cluster decoder's settings, and the standalone
    ``decoder(llr, pcm, s, bs)`` call of `OSD0_Decoder` served by `fgnn_lsd` on the matrix as given (no row basis; dependent rows are
    fine).  ``max_pivots`` caps the pivots per sample (None: what the kernel's LDS holds, `TannerGraph.lsd_max_pivots`), ``max_rounds``
    the growth rounds (None: no limit).  A sample that comes back with found = 0 (a cap was hit, or the syndrome is not in the image)
    is re-solved by OSD-0 when ``fallback="osd0"`` — the basis over all rows that `_graph_of` installs serves only that — or left as
    the read-out of its pivots when ``fallback=None``.  ``last_stats`` [bs, 4] int32 = (found, rounds, columns, pivots) of the last
    standalone call."""

    def __init__(self, n, max_pivots=None, max_rounds=None, fallback="osd0", device=None):
        super().__init__(n, device)
        if fallback not in FALLBACKS:
            raise ValueError(f"fallback must be one of {FALLBACKS}")
        self.max_pivots = 0 if max_pivots is None else int(max_pivots)
        self.max_rounds = 0 if max_rounds is None else int(max_rounds)
        if self.max_pivots < 0 or self.max_rounds < 0:
            raise ValueError("max_pivots and max_rounds must be >= 0")
        self.fallback = fallback
        self.last_stats = None

    def _solve(self, g, synd, e_hat, llr):
        stats = _fresh_stats(g, int(synd.shape[0]))
        g.lsd(0, synd, e_hat, llr_bin=llr, max_pivots=self.max_pivots, max_rounds=self.max_rounds, stats=stats[0])
        self.last_stats = stats[0]
        if self.fallback == "osd0":
            index, nact = _missed(g, stats)
            if nact:
                _run_osd0(g, self._ws, 0, synd, e_hat, llr_bin=llr, index=index, nact=nact)


class BP4_LSD_Model(ShardedModel):
    """``BP4_LSD_Model(code, bp4_decoder, lsd_decoder)``; ``model(batch_size, p)`` → ``(zeros_like(ls_hat), ls_hat)`` as
    `BP4_OSD_Model`: BP4 on every sample, the samples whose estimate misses the syndrome compacted and both halves re-solved by LSD on
    the full hx / hz from the binary reliabilities of their BP marginals.  Samples LSD returns with found = 0 on either side are
    compacted again and handed to OSD-0 (``lsd_decoder.fallback == "osd0"``: the row bases ``code.pivot_hx`` / ``code.pivot_hz`` are
    installed) or left as they are (``fallback=None``).  ``last_num_lsd`` / ``last_num_fallback`` count the two lists, ``last_stats``
    [2, bs, 4] holds the LSD stats of side 0 (hx, z_hat) and side 1 (hz, x_hat)."""

    def __init__(self, code, bp4_decoder, lsd_decoder, *, seed=0x5EED, rank=0, world_size=1):
        self.code, self.bp4_decoder, self.lsd_decoder = code, bp4_decoder, lsd_decoder
        self.graph = bp4_decoder.graph
        if lsd_decoder.fallback == "osd0":
            self.graph.set_basis(0, code.pivot_hx)
            self.graph.set_basis(1, code.pivot_hz)
        self.channel = Pauli(self.graph, seed=seed)
        self._shard(self.channel.seed, rank, world_size)
        self.last_num_lsd = self.last_num_fallback = 0
        self.last_stats = None
        self._ws = _OsdWorkspace()  # used only by the fallback, for a basis the LDS-resident OSD kernel refuses

    def decode(self, batch_size, p):
        B, g, d, l = int(batch_size), self.graph, self.bp4_decoder, self.lsd_decoder
        ex, ez = self.channel(B, float(p), self._take(B))
        sx, sz = g.syndrome(ex, ez)
        decode = g.bp4_decode_layered if getattr(d, "schedule", "flooding") == "layered" else g.bp4_decode
        out = decode(sx, sz, d.num_iter, d.cn_type, d.normalization_factor, llr_const=depolarizing_llr(p), want_logits=False)
        x_hat, z_hat = out["x_hat"], out["z_hat"]
        _, _, flags = g.residual(ex, ez, x_hat, z_hat, want_arrays=False)  # bit 0 = syndrome missed
        index, nact = g.compact(flags, 1)
        self.last_num_lsd, self.last_num_fallback = nact, 0
        self.last_stats = stats = _fresh_stats(g, B, 2)
        if nact:
            kw = dict(marg=out["llr"], index=index, nact=nact, max_pivots=l.max_pivots, max_rounds=l.max_rounds)
            g.lsd(0, sx, z_hat, stats=stats[0], **kw)
            g.lsd(1, sz, x_hat, stats=stats[1], **kw)
            if l.fallback == "osd0":
                index2, nact2 = _missed(g, stats)
                self.last_num_fallback = nact2
                if nact2:
                    _run_osd0(g, self._ws, 0, sx, z_hat, marg=out["llr"], index=index2, nact=nact2)
                    _run_osd0(g, self._ws, 1, sz, x_hat, marg=out["llr"], index=index2, nact=nact2)
        return dict(noise_x=ex, noise_z=ez, x_hat=x_hat, z_hat=z_hat)

    def __call__(self, batch_size, ebno_db=None, **kw):
        o = self.decode(batch_size, kw.get("p", ebno_db))
        ls_hat, _ = self.graph.residual_rows(ROWS_LZ, ROWS_LX, o["noise_x"], o["noise_z"], o["x_hat"], o["z_hat"])
        return torch.zeros_like(ls_hat), ls_hat

    call = __call__


class BP2_LSD_Model(ShardedModel):
    """``BP2_LSD_Model(pcm, logical_pcm, bp2_decoder, lsd_decoder)``; ``model(batch_size, p)`` → ``(zeros_like(ls_hat), ls_hat[bs,
    rows(logical_pcm)])`` as `BP2_OSD_Model` with LSD on the full ``pcm`` in OSD's place: no basis and no pivots are passed in (the
    fallback's OSD-0 runs on all rows of ``pcm``, which may be dependent)."""

    def __init__(self, pcm, logical_pcm, bp2_decoder, lsd_decoder, *, seed=0x5EED, rank=0, world_size=1):
        from .decoding import _adopt_bit_layers, _binary_graph
        self.pcm, self.logical_pcm, self.bp2_decoder, self.lsd_decoder = pcm, logical_pcm, bp2_decoder, lsd_decoder
        self.graph = _binary_graph(pcm, logical_pcm, bp2_decoder.graph.device)
        _adopt_bit_layers(self.graph, bp2_decoder)
        if lsd_decoder.fallback == "osd0":
            self.graph.set_basis(0, np.arange(self.graph.m_x, dtype=np.int32))
        self._shard(seed, rank, world_size)
        self.last_num_lsd = self.last_num_fallback = 0
        self.last_stats = None
        self._ws = _OsdWorkspace()

    def __call__(self, batch_size, ebno_db=None, **kw):
        p = float(kw.get("p", ebno_db))
        B, g, d, l = int(batch_size), self.graph, self.bp2_decoder, self.lsd_decoder
        noise = g.bsc_noise(self.seed, p, self._take(B), B)
        zeros = torch.zeros_like(noise)
        synd, _ = g.syndrome(zeros, noise)
        soft, noise_hat = _bp2_stage(g, d, synd, llr_const=bsc_logit(p), B=B)
        _, _, flags = g.residual(noise, zeros, noise_hat, zeros, want_arrays=False)
        index, nact = g.compact(flags, 1)
        self.last_num_lsd, self.last_num_fallback = nact, 0
        self.last_stats = stats = _fresh_stats(g, B)
        if nact:
            llr = (-soft).contiguous()  # llr_hat = -decoder output, as BP2_OSD_Model
            g.lsd(0, synd, noise_hat, llr_bin=llr, index=index, nact=nact, max_pivots=l.max_pivots, max_rounds=l.max_rounds,
                  stats=stats[0])
            if l.fallback == "osd0":
                index2, nact2 = _missed(g, stats)
                self.last_num_fallback = nact2
                if nact2:
                    _run_osd0(g, self._ws, 0, synd, noise_hat, llr_bin=llr, index=index2, nact=nact2)
        _, ls_hat, _ = g.residual(noise, zeros, noise_hat, zeros, want_arrays=True)
        ls_hat = ls_hat[:, :g.rows_hxp].contiguous()
        return torch.zeros_like(ls_hat), ls_hat

    call = __call__
