"""OSD-0 post-processing and the BP4+OSD evaluation model on MI355X — SURVEY.md §8(f) rank 2.

Drop-ins for `OSD0_Decoder` and `BP4_OSD_Model` of /root/reference sionna/fec/ldpc/bp_osd.py:8-191.
"""
import weakref

import numpy as np
import torch

from ._frontend import ShardedModel, bsc_logit, depolarizing_llr
from ._lib import ROWS_LX, ROWS_LZ
from .decoding import _bp2_stage
from .feedback_gnn import Pauli

_SEARCH = "osd_cs"  # fgnn_osd_resident of a search method asks whether fgnn_osd (the kernel every osd() call runs) takes the basis


class _OsdWorkspace:
    """The device workspace of the OSD path beyond LDS (`fgnn_osd_ws`), taken only for a basis the LDS-resident kernels refuse: one
    tensor per owner, grown on demand (the default slot count of the largest request so far)."""

    def __init__(self):
        self.buf = None

    def get(self, g, side, method, order):
        self.buf = g.osd_workspace(side, method, order, out=self.buf)
        return self.buf


def _run_osd0(g, ws, side, synd, e_hat, **kw):
    """OSD-0 of side `side`: `fgnn_osd0` where it takes the basis, else `fgnn_osd_ws` on the owner's workspace."""
    if g.osd_resident(side, "osd0"):
        g.osd0(side, synd, e_hat, **kw)
    else:
        g.osd_ws(side, synd, e_hat, "osd0", 0, workspace=ws.get(g, side, "osd0", 0), **kw)


def _run_osd(g, ws, side, synd, e_hat, method, order, **kw):
    """OSD-E / OSD-CS of side `side`: `fgnn_osd` where it takes the basis, else `fgnn_osd_ws` on the owner's workspace."""
    if g.osd_resident(side, _SEARCH):
        g.osd(side, synd, e_hat, method, order, **kw)
    else:
        g.osd_ws(side, synd, e_hat, method, order, workspace=ws.get(g, side, method, order), **kw)


class _StandaloneOSD:
    """The reference's standalone ``decoder(llr, pcm, s, bs)`` call (bp_osd.py:47-77) over one device graph per row basis; the
    subclass says which kernel solves it (`_solve`)."""

    MAX_CACHED = 4  # device graphs kept (a script alternates the hx and the hz basis, bp_osd.py:147-157: two)

    def __init__(self, n, device=None):
        self.n = int(n)
        self._device = device
        self._graphs = {}     # basis bytes -> device graph with the basis installed (a caller reuses its bases for every batch)
        self._seen = {}       # identity of a pcm tensor already resolved (storage pointer, shape, strides, version) -> its graph
        self._seen_refs = {}  # same keys -> weak reference to that tensor: a hit needs the very same live tensor (a freed one's
        #                       storage may come back from the allocator for a different matrix with an identical key)
        self._ws = _OsdWorkspace()  # used only for a basis the LDS-resident kernels refuse

    def _graph_of(self, basis):
        from .decoding import _binary_graph
        key = (basis.shape, basis.tobytes())
        g = self._graphs.pop(key, None)
        if g is None:
            g = _binary_graph(basis, None, self._device)
            g.set_basis(0, np.arange(basis.shape[0], dtype=np.int32))
        self._graphs[key] = g  # most recently used last
        while len(self._graphs) > self.MAX_CACHED:
            old = next(iter(self._graphs))
            self._seen = {k: v for k, v in self._seen.items() if v is not self._graphs[old]}
            self._seen_refs = {k: r for k, r in self._seen_refs.items() if k in self._seen}
            del self._graphs[old]
        return g

    def _resolve(self, pcm):
        pcm_t = torch.as_tensor(pcm)
        ident = (pcm_t.untyped_storage().data_ptr(), pcm_t.storage_offset(), tuple(pcm_t.shape), tuple(pcm_t.stride()), pcm_t._version,
                 pcm_t.dtype, str(pcm_t.device))
        # only a torch tensor has a version counter that sees in-place writes; anything else (a NumPy array ...) is resolved by content
        is_tensor = isinstance(pcm, torch.Tensor)
        g = None
        if is_tensor:
            ref = self._seen_refs.get(ident)
            if ref is not None and ref() is pcm:
                g = self._seen.get(ident)
        if g is None:
            if pcm_t.dim() == 3:
                tiled = pcm_t.shape[0] <= 1 or pcm_t.stride(0) == 0 or bool((pcm_t == pcm_t[:1]).all())
                if not tiled:
                    raise NotImplementedError(f"{type(self).__name__}: one row basis per call (the reference tiles the same matrix over "
                                              "the batch)")
                pcm_t = pcm_t[0]
            basis = np.ascontiguousarray(pcm_t.cpu().numpy() != 0, dtype=np.uint8)
            if basis.shape[1] != self.n:
                raise ValueError("pcm must have n columns")
            g = self._graph_of(basis)
            if len(self._seen) > 64:
                self._seen.clear()
                self._seen_refs.clear()
            if is_tensor:
                self._seen[ident] = g
                self._seen_refs[ident] = weakref.ref(pcm)
        return g

    def _solve(self, g, synd, e_hat, llr):
        raise NotImplementedError

    def __call__(self, llr, pcm, s, bs=None):
        """The reference's standalone call (bp_osd.py:47-77): ``llr [bs, n]`` binary reliabilities (sorted ascending: the least
        reliable "no error" positions become the pivots), ``pcm [bs, rank, n]`` the row basis tiled over the batch (the
        reference's models tile one matrix, :147-150; this implementation requires that — or takes a plain ``[rank, n]`` matrix),
        ``s [rank, bs]`` the syndrome of those rows → ``e_hat [bs, n]`` bool with ``pcm e_hat = s`` on the most reliable basis.
        The rows may be dependent (a full ``hx`` is fine): rows that reduce to zero are ignored, and ``pcm e_hat = s`` holds
        whenever ``s`` lies in the row space of ``pcm`` (for any ``s`` that comes from an error).
        Ties in the sort keep qubit order (tf.argsort leaves them unspecified).

        Host-side cost: the first call with a given ``pcm`` tensor checks that it is one matrix tiled over the batch (skipped for an
        expanded, stride-0 batch dimension), copies it to the host once and builds (or finds) its device graph; later calls with the
        SAME live tensor (same object, storage, shape, strides and version counter) go straight to the kernel — no device
        synchronisation, no copy, no hash."""
        g = self._resolve(pcm)
        rank = g.m_x
        llr = torch.as_tensor(llr, device=g.device).to(torch.float32).contiguous()
        B = int(llr.shape[0])
        if bs is not None and int(bs) != B:
            raise ValueError("bs must equal the leading dimension of llr")
        synd = (torch.as_tensor(s, device=g.device).to(torch.int64) & 1).to(torch.uint8).t().contiguous()
        if tuple(synd.shape) != (B, rank):
            raise ValueError(f"s must have shape [{rank}, {B}]")
        e_hat = torch.zeros((B, self.n), dtype=torch.uint8, device=g.device)
        self._solve(g, synd, e_hat, llr)
        return e_hat.bool()

    call = __call__


class OSD0_Decoder(_StandaloneOSD):
    """Order-0 ordered-statistics decoder (bp_osd.py:8-77).  Inside `BP4_OSD_Model` / `BP2_OSD_Model` the row basis lives in the
    model's device graph (`fgnn_graph_set_basis`) and only the BP failures are re-solved; the reference's standalone
    ``decoder(llr, pcm, s, bs)`` is served by `__call__` through the same HIP kernel (`fgnn_osd0`; `fgnn_osd_ws` for a basis beyond LDS)."""

    def _solve(self, g, synd, e_hat, llr):
        _run_osd0(g, self._ws, 0, synd, e_hat, llr_bin=llr)


class OSD_Decoder(_StandaloneOSD):
    """Higher-order OSD with the ``osd_method`` / ``osd_order`` of ``ldpc.bposd_decoder`` (examples/OSD.ipynb cell 5): "osd_cs"
    (combination sweep: every weight-1 and the weight-2 vectors on the ``osd_order`` least reliable non-pivot columns), "osd_e"
    (exhaustive over ``osd_order`` <= 16 columns) or "osd0".  Candidate list, cost and tie rule: include/fgnn.h, `fgnn_osd`.  Passed to
    `BP4_OSD_Model` / `BP2_OSD_Model` it replaces their OSD-0 step; standalone it offers the same ``__call__`` as `OSD0_Decoder`."""

    def __init__(self, n, osd_method="osd_cs", osd_order=7, device=None):
        super().__init__(n, device)
        from .graph import osd_method_id
        self.osd_method, self.osd_order = str(osd_method), int(osd_order)
        self.method_id = osd_method_id(self.osd_method)
        limit = {0: None, 1: 16, 2: 64}[self.method_id]
        if self.osd_order < 0 or (limit is not None and self.osd_order > limit):
            raise ValueError(f"osd_order must be in 0..{limit} for {self.osd_method}")

    def _solve(self, g, synd, e_hat, llr):
        _run_osd(g, self._ws, 0, synd, e_hat, self.method_id, self.osd_order, llr_bin=llr)


def _search_of(osd_decoder):
    """(method, order) when the models' osd_decoder asks for a higher-order search (it carries osd_method / osd_order), else None."""
    method = getattr(osd_decoder, "osd_method", None)
    return None if method is None else (method, int(getattr(osd_decoder, "osd_order", 0)))


def _improved(chosen):
    """Samples whose winner is not candidate 0, over one or more `chosen` buffers (zero-filled, so untouched entries count as 0)."""
    hit = chosen[0] != 0
    for c in chosen[1:]:
        hit |= c != 0
    return int(hit.sum())


class BP4_OSD_Model(ShardedModel):
    """``BP4_OSD_Model(code, bp4_decoder, osd_decoder)``; ``model(batch_size, p)`` → ``(zeros_like(ls_hat), ls_hat)`` with
    ``ls_hat[bs, rows(lz)+rows(lx)] = [lz·x_diff ; lx·z_diff]`` (bp_osd.py:159-191).  BP4 runs on every sample with
    ``llr = log(3(1-p)/p)`` (:106); the samples whose estimate misses the syndrome get both halves re-solved by OSD-0 from
    the binary reliabilities of their BP marginals (:117-131, :138-157)."""

    def __init__(self, code, bp4_decoder, osd_decoder, *, seed=0x5EED, rank=0, world_size=1):
        self.code, self.bp4_decoder, self.osd_decoder = code, bp4_decoder, osd_decoder
        self.graph = bp4_decoder.graph
        self.graph.set_basis(0, code.pivot_hx)
        self.graph.set_basis(1, code.pivot_hz)
        self.channel = Pauli(self.graph, seed=seed)
        self._shard(self.channel.seed, rank, world_size)
        self.last_num_osd = 0
        self.last_osd_improved = 0  # processed samples whose OSD winner is not the OSD-0 solution (OSD_Decoder only)
        self._ws = _OsdWorkspace()  # used only for a basis the LDS-resident kernels refuse

    def decode(self, batch_size, p):
        B, g, d = int(batch_size), self.graph, self.bp4_decoder
        ex, ez = self.channel(B, float(p), self._take(B))
        sx, sz = g.syndrome(ex, ez)
        decode = g.bp4_decode_layered if getattr(d, "schedule", "flooding") == "layered" else g.bp4_decode
        out = decode(sx, sz, d.num_iter, d.cn_type, d.normalization_factor, llr_const=depolarizing_llr(p), want_logits=False)
        x_hat, z_hat = out["x_hat"], out["z_hat"]
        _, _, flags = g.residual(ex, ez, x_hat, z_hat, want_arrays=False)  # bit 0 = syndrome missed = `err` (:117-120)
        index, nact = g.compact(flags, 1)
        self.last_num_osd = nact
        self.last_osd_improved = 0
        search = _search_of(self.osd_decoder)
        if nact and search is not None:
            cz, cx = torch.zeros((2, B), dtype=torch.int32, device=g.device)
            _run_osd(g, self._ws, 0, sx, z_hat, *search, marg=out["llr"], index=index, nact=nact, chosen=cz)
            _run_osd(g, self._ws, 1, sz, x_hat, *search, marg=out["llr"], index=index, nact=nact, chosen=cx)
            self.last_osd_improved = _improved([cz, cx])
        elif nact:
            _run_osd0(g, self._ws, 0, sx, z_hat, marg=out["llr"], index=index, nact=nact)  # z_hat_osd from hx, osd_llrz (:155)
            _run_osd0(g, self._ws, 1, sz, x_hat, marg=out["llr"], index=index, nact=nact)  # x_hat_osd from hz, osd_llrx (:156)
        return dict(noise_x=ex, noise_z=ez, x_hat=x_hat, z_hat=z_hat)

    def __call__(self, batch_size, ebno_db=None, **kw):
        o = self.decode(batch_size, kw.get("p", ebno_db))
        ls_hat, _ = self.graph.residual_rows(ROWS_LZ, ROWS_LX, o["noise_x"], o["noise_z"], o["x_hat"], o["z_hat"])
        return torch.zeros_like(ls_hat), ls_hat

    call = __call__


class BP2_OSD_Model(ShardedModel):
    """``BP2_OSD_Model(pcm, pcm_basis, pivot_pcm, logical_pcm, bp2_decoder, osd_decoder)``; ``model(batch_size, p)`` →
    ``(zeros_like(ls_hat), ls_hat[bs, rows(logical_pcm)])`` (bp_osd.py:194-273): BSC(p) noise, binary syndrome BP with soft
    output, OSD-0 on the samples whose estimate misses the syndrome, ``ls_hat = logical_pcm·(noise xor estimate)``."""

    def __init__(self, pcm, pcm_basis, pivot_pcm, logical_pcm, bp2_decoder, osd_decoder, *, seed=0x5EED, rank=0, world_size=1):
        from .decoding import _adopt_bit_layers, _binary_graph
        self.pcm, self.logical_pcm, self.bp2_decoder, self.osd_decoder = pcm, logical_pcm, bp2_decoder, osd_decoder
        self.graph = _binary_graph(pcm, logical_pcm, bp2_decoder.graph.device)
        _adopt_bit_layers(self.graph, bp2_decoder)
        self.graph.set_basis(0, pivot_pcm)
        self._shard(seed, rank, world_size)
        self.last_num_osd = 0
        self.last_osd_improved = 0  # processed samples whose OSD winner is not the OSD-0 solution (OSD_Decoder only)
        self._ws = _OsdWorkspace()  # used only for a basis the LDS-resident kernels refuse

    def __call__(self, batch_size, ebno_db=None, **kw):
        p = float(kw.get("p", ebno_db))
        B, g, d = int(batch_size), self.graph, self.bp2_decoder
        noise = g.bsc_noise(self.seed, p, self._take(B), B)
        zeros = torch.zeros_like(noise)
        synd, _ = g.syndrome(zeros, noise)
        soft, noise_hat = _bp2_stage(g, d, synd, llr_const=bsc_logit(p), B=B)  # (:216)
        _, _, flags = g.residual(noise, zeros, noise_hat, zeros, want_arrays=False)
        index, nact = g.compact(flags, 1)
        self.last_num_osd = nact
        self.last_osd_improved = 0
        search = _search_of(self.osd_decoder)
        if nact and search is not None:
            chosen = torch.zeros(B, dtype=torch.int32, device=g.device)
            _run_osd(g, self._ws, 0, synd, noise_hat, *search, llr_bin=(-soft).contiguous(), index=index, nact=nact, chosen=chosen)
            self.last_osd_improved = _improved([chosen])
        elif nact:
            _run_osd0(g, self._ws, 0, synd, noise_hat, llr_bin=(-soft).contiguous(), index=index, nact=nact)  # llr_hat = -decoder output (:225)
        _, ls_hat, _ = g.residual(noise, zeros, noise_hat, zeros, want_arrays=True)
        ls_hat = ls_hat[:, :g.rows_hxp].contiguous()
        return torch.zeros_like(ls_hat), ls_hat

    call = __call__
