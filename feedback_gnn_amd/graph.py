"""Device-resident Tanner graphs of a CSS code and thin torch-tensor wrappers over the C ABI.

`TannerGraph` owns one `fgnn_graph` handle (include/fgnn.h).  PyTorch-ROCm is used only for
device memory and streams: every method takes/returns torch tensors that live on the graph's
device, passes their `data_ptr()` and the current HIP stream to the library, and never touches
the data on the host.  Layouts are the library's codeword-major ones (fgnn.h "Conventions").
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import CN_TYPES, check


def _coo(mat):
    r, c = np.nonzero(np.asarray(mat))
    return np.ascontiguousarray(r, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32)


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# osd_method names of ldpc.bposd_decoder (examples/OSD.ipynb cell 5) -> FGNN_OSD_0 / FGNN_OSD_E / FGNN_OSD_CS of include/fgnn.h
OSD_METHODS = {"osd0": 0, "osd_0": 0, "osd_e": 1, "osde": 1, "exhaustive": 1, "osd_cs": 2, "osdcs": 2, "combination_sweep": 2}


def osd_method_id(method):
    if isinstance(method, str):
        key = method.lower()
        if key not in OSD_METHODS:
            raise ValueError(f"unknown OSD method {method!r} (one of {sorted(OSD_METHODS)})")
        return OSD_METHODS[key]
    return int(method)


def _resolve_device(device):
    """torch.device with an explicit index: None and a bare "cuda" mean torch's CURRENT device (not device 0)."""
    device = torch.device("cuda" if device is None else device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


REDUCE_OPS = {"sum": 0, "mean": 1, "max": 2, "min": 3}
ACTIVATIONS = {None: 0, "linear": 0, "tanh": 1, "relu": 2, "sigmoid": 3}
SHIPPED_GNN_CONFIG = (20, 40, 2, "mean", "tanh", True)


def gnn_weight_shapes(num_msg_dims, num_hidden_units, num_mlp_layers, use_bias=True):
    """Shapes of Feedback_GNN.get_weights() (feedback_gnn.py:110-128): _llr_inv_embed, vn_msg_mlp_x, vn_msg_mlp_z, vn_embed_mlp."""
    D, H, L = int(num_msg_dims), int(num_hidden_units), int(num_mlp_layers)
    dense = [(H if L > 1 else 2 * D + 3, 3)]
    for _ in range(2):
        dense += [(4 if l == 0 else H, D if l == L - 1 else H) for l in range(L)]
    dense += [(2 * D + 3 if l == 0 else H, H) for l in range(L - 1)]
    shapes = []
    for k, j in dense:
        shapes.append((k, j))
        if use_bias:
            shapes.append((j,))
    return shapes


class GnnWeights:
    """Device copy of one feedback GNN's weight arrays (fgnn_weights).  ``config`` = (num_msg_dims, num_hidden_units,
    num_mlp_layers, reduce_op, activation, use_bias); the shipped configuration takes the MFMA kernel, any other one the
    runtime-shaped kernel (fgnn_weights_create_general)."""

    def __init__(self, arrays, device, config=SHIPPED_GNN_CONFIG, force_general=False):
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        D, H, L, red, act, bias = config
        if red not in REDUCE_OPS:
            raise ValueError("unknown reduce operation")  # feedback_gnn.py:148
        if act not in ACTIVATIONS:
            raise NotImplementedError(f"activation {act!r}: the HIP kernels implement {sorted(k for k in ACTIVATIONS if k)}")
        shapes = gnn_weight_shapes(D, H, L, bias)
        if [a.shape for a in arrays] != shapes:
            raise ValueError(f"feedback-GNN weights must have shapes {shapes}, got {[a.shape for a in arrays]}")
        self.arrays = arrays
        self.config = (int(D), int(H), int(L), red, act, bool(bias))
        self.device = _resolve_device(device)
        self.general = force_general or self.config != SHIPPED_GNN_CONFIG
        ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
        h = C.c_void_p()
        if self.general:
            cfg = (C.c_int * 6)(int(D), int(H), int(L), REDUCE_OPS[red], ACTIVATIONS[act], int(bool(bias)))
            check(_lib.lib().fgnn_weights_create_general(cfg, ptrs, len(arrays), self.device.index, C.byref(h)))
        else:
            check(_lib.lib().fgnn_weights_create(ptrs, self.device.index, C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().fgnn_weights_destroy(self.handle)
        except Exception:
            pass


class TannerGraph:
    """hx/hz Tanner graphs + soft-syndrome row sets + hx_perp/hz_perp of one CSS code on one GPU.

    stage_one=True installs pcm_x_perp = hz, pcm_z_perp = hx as the soft-syndrome rows
    (reference decoding_q.py:35-37), otherwise code.hx_perp / code.hz_perp (:33-34).
    """

    def __init__(self, code, stage_one=True, device=None):
        if device is not None and torch.device(device).type != "cuda":
            raise _lib.FgnnError("the BP4/feedback-GNN decoder runs on a HIP device only (no CPU fallback)")
        if not torch.cuda.is_available():
            raise _lib.FgnnError("no HIP device: the BP4/feedback-GNN decoder has no CPU fallback")
        self.device = _resolve_device(device)
        L = _lib.lib()
        self.code = code
        hx, hz = np.asarray(code.hx), np.asarray(code.hz)
        self.n = int(hx.shape[1])
        self.m_x, self.m_z = int(hx.shape[0]), int(hz.shape[0])
        rx, cx = _coo(hx)
        rz, cz = _coo(hz)
        self.E_x, self.E_z = len(rx), len(rz)
        h = C.c_void_p()
        check(L.fgnn_graph_create(self.n, self.m_x, self.m_z, self.E_x, _np_ptr(rx), _np_ptr(cx), self.E_z, _np_ptr(rz),
                                  _np_ptr(cz), self.device.index, C.byref(h)))
        self.handle = h
        self.gnn_factored = False  # the library default: the reference's association, one Dense per edge (FGNN_OPT_GNN_FACTORED is opt-in)
        self.gnn_stream = True  # the library default (FGNN_OPT_GNN_STREAM)
        self.bp4_shared_lse = False  # the library default: one log-sum-exp per edge (FGNN_OPT_BP4_SHARED_LSE is opt-in)
        self.stage_one = bool(stage_one)
        xp, zp = (hz, hx) if stage_one else (np.asarray(code.hx_perp), np.asarray(code.hz_perp))
        self.rows_xp, self.rows_zp = int(xp.shape[0]), int(zp.shape[0])
        self.rows_hxp, self.rows_hzp = int(code.hx_perp.shape[0]), int(code.hz_perp.shape[0])
        self.rows_lx, self.rows_lz = int(np.asarray(code.lx).shape[0]), int(np.asarray(code.lz).shape[0])
        for which, mat in ((0, xp), (1, zp), (2, code.hx_perp), (3, code.hz_perp), (4, code.lx), (5, code.lz)):
            r, c = _coo(mat)
            check(L.fgnn_graph_set_rows(self.handle, which, int(np.asarray(mat).shape[0]), len(r), _np_ptr(r), _np_ptr(c)))

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().fgnn_graph_destroy(self.handle)
        except Exception:
            pass

    # ---- introspection ------------------------------------------------------------------------
    def info(self):
        buf = (C.c_int32 * 16)()
        check(_lib.lib().fgnn_graph_info(self.handle, buf))
        keys = ("n", "m_x", "m_z", "E_x", "E_z", "threads_per_codeword", "codewords_per_block", "lds_bytes_per_block",
                "regular", "device", "dv_x", "dv_z", "dc")
        return dict(zip(keys, list(buf)))

    def set_launch(self, threads_per_codeword=0, codewords_per_block=0):
        check(_lib.lib().fgnn_graph_set_launch(self.handle, int(threads_per_codeword), int(codewords_per_block)))

    def set_saturation_shortcut(self, on=True):
        """Exact wave-uniform shortcut for saturated nodes in the regular BP4 kernel (default on; same results)."""
        check(_lib.lib().fgnn_graph_set_option(self.handle, 1, int(bool(on))))

    def set_fixed_point_exit(self, on=True):
        """Exact early exit of converged codewords (FGNN_OPT_FIXED_POINT_EXIT; only acts with the saturation shortcut on)."""
        check(_lib.lib().fgnn_graph_set_option(self.handle, 2, int(bool(on))))

    def set_hw_transcendentals(self, on=True):
        """OPT-IN, not bit-exact (FGNN_OPT_HW_TRANSCENDENTALS): boxplus-phi decodes run on v_exp_f32 / v_log_f32 in the fixed
        dataflow, phi's clip points pinned to the reference's known-answer values (same saturated fixed point as the exact kernel,
        different bits in the transient).  Off by default; no parity test and no headline number uses it."""
        check(_lib.lib().fgnn_graph_set_option(self.handle, 3, int(bool(on))))

    def set_gnn_factored(self, on=True):
        """OPT-IN re-association (FGNN_OPT_GNN_FACTORED, default off = feedback_gnn.py:175-184 term by term): the X/Y/Z part of the first
        Dense once per qubit and side, one last Dense on the edge-summed activations.  Same real-number function, float32 rounding differs
        (<= 5e-7 on the output): statistically the same decoder, not the reference's operation sequence."""
        check(_lib.lib().fgnn_graph_set_option(self.handle, 4, int(bool(on))))
        self.gnn_factored = bool(on)

    def set_gnn_stream(self, on=True):
        """Feedback GNN of a regular graph on the streaming VALU kernel (FGNN_OPT_GNN_STREAM): True (default) = wherever it is the
        faster kernel (launches of 4 096 codewords or more), "always" = every launch, False = never
        (MFMA-tile kernel).  The same float operations in the same order: bit-identical results.  "always" also moves `gnn_bp4_decode`
        on a (3,3,6)-regular graph to its streaming kernel, which is bit-identical and ~35 % SLOWER than its MFMA tiles (the tested
        second implementation, include/fgnn.h option 6); True / False leave GNN_BP4 on the MFMA tiles."""
        value = 2 if on == "always" else int(bool(on))
        check(_lib.lib().fgnn_graph_set_option(self.handle, 6, value))
        self.gnn_stream = "always" if value == 2 else bool(value)

    def set_bp4_shared_lse(self, on=True):
        """OPT-IN re-association (FGNN_OPT_BP4_SHARED_LSE, default off = decoding_q.py:254-273 term by term): the (a - b)-dependent part
        of the qubit update's log-sum-exp formed once per qubit and side instead of once per edge — same real-number function, 4 instead
        of 8 exp/log pairs per qubit and iteration, v->c messages move by <= 4 ulp of the totals per update: statistically the same
        decoder, not the reference's operation sequence."""
        check(_lib.lib().fgnn_graph_set_option(self.handle, 5, int(bool(on))))
        self.bp4_shared_lse = bool(on)

    def force_generic(self, on=True):
        """Testing hook: run the runtime-degree kernel even on a degree-regular graph."""
        check(_lib.lib().fgnn_graph_force_generic(self.handle, int(bool(on))))

    def profile_enable(self, max_launches):
        """Record HIP events around every BP4 launch (0 disables)."""
        check(_lib.lib().fgnn_profile_enable(self.handle, int(max_launches)))
        self._prof_cap = int(max_launches)

    def profile_read(self):
        """[(ms, num_iter, batch), ...] of the BP4 launches since the last read."""
        cap = max(1, getattr(self, "_prof_cap", 0))
        ms = np.zeros(cap, np.float32)
        it = np.zeros(cap, np.int32)
        bt = np.zeros(cap, np.int32)
        cnt = C.c_int32(0)
        check(_lib.lib().fgnn_profile_read(self.handle, _np_ptr(ms), _np_ptr(it), _np_ptr(bt), cap, C.byref(cnt)))
        return [(float(ms[i]), int(it[i]), int(bt[i])) for i in range(cnt.value)]

    def edges(self, side):
        """Canonical (qubit, check)-sorted edge list of hx (side 0) or hz (side 1): (chk, var)."""
        E = self.E_x if side == 0 else self.E_z
        chk = np.empty(E, np.int32)
        var = np.empty(E, np.int32)
        check(_lib.lib().fgnn_graph_edges(self.handle, side, _np_ptr(chk), _np_ptr(var)))
        return chk, var

    # ---- helpers ----------------------------------------------------------------------------------
    def _chk(self, t, shape, dtype, name):
        if t.device != self.device:
            raise ValueError(f"{name} must live on {self.device}, got {t.device}")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.contiguous()

    def _chk_out(self, t, shape, dtype, name):
        """A buffer the library writes in place: validated like an input, but a non-contiguous view is an error (a silent copy
        would receive the result instead of the caller's tensor)."""
        self._chk(t, shape, dtype, name)
        if not t.is_contiguous():
            raise ValueError(f"{name} is written in place and must be contiguous")
        return t

    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    # ---- the input / output frame of the wrappers below: each checks in the order its arguments are listed ----
    def _opt(self, t, shape, dtype, name):
        """`_chk` of an input that may be omitted."""
        return None if t is None else self._chk(t, shape, dtype, name)

    def _opt_any(self, t, dtype, name):
        """An input of any shape that may be omitted: checked for device and dtype only."""
        return None if t is None else self._chk(t, tuple(t.shape), dtype, name)

    @staticmethod
    def _cn(cn_type):
        if cn_type not in CN_TYPES:
            raise ValueError("Unknown node type.")
        return CN_TYPES[cn_type]

    def _syndromes_in(self, synd_x, synd_z):
        """(B, synd_x, synd_z) of a call that needs both syndromes."""
        B = int(synd_x.shape[0])
        return B, self._chk(synd_x, (B, self.m_x), torch.uint8, "synd_x"), self._chk(synd_z, (B, self.m_z), torch.uint8, "synd_z")

    def _quaternary_in(self, synd_x, synd_z, llr_ch, B, also=(), missing="B is needed when neither syndromes nor llr_ch are given"):
        """(B, synd_x, synd_z, llr_ch) of a step-loop decoder: each may be None (a syndrome: all-zero; llr_ch: one constant); ``also``
        are further inputs that can give the batch size: the last one given does, else ``B``, else a ValueError says ``missing``.
        The checks are written out, not passed through `_opt`: this runs on every decode call."""
        for t in (synd_x, synd_z, llr_ch, *also):
            if t is not None:
                B = int(t.shape[0])
        if B is None:
            raise ValueError(missing)
        if synd_x is not None:
            synd_x = self._chk(synd_x, (B, self.m_x), torch.uint8, "synd_x")
        if synd_z is not None:
            synd_z = self._chk(synd_z, (B, self.m_z), torch.uint8, "synd_z")
        if llr_ch is not None:
            llr_ch = self._chk(llr_ch, (B, 3, self.n), torch.float32, "llr_ch")
        return B, synd_x, synd_z, llr_ch

    def _binary_in(self, synd, llr_ch, B):
        """(B, synd, llr_ch) of a decoder of the hx graph alone: the syndrome's batch size wins, then ``B``, then llr_ch's."""
        if synd is not None:
            B = int(synd.shape[0])
            synd = self._chk(synd, (B, self.m_x), torch.uint8, "syndrome")
        if llr_ch is not None:
            B = int(llr_ch.shape[0]) if B is None else B
            llr_ch = self._chk(llr_ch, (B, self.n), torch.float32, "llr_ch")
        return B, synd, llr_ch

    def _gnn_in(self, llr, logit_hx, logit_hz, synd_x, synd_z):
        """(B, llr, logit_hx, logit_hz, synd_x, synd_z) of the feedback GNN."""
        B = int(llr.shape[0])
        return (B, self._chk(llr, (B, 3, self.n), torch.float32, "llr"), self._chk(logit_hx, (B, self.m_x), torch.float32, "logit_hx"),
                self._chk(logit_hz, (B, self.m_z), torch.float32, "logit_hz"), self._chk(synd_x, (B, self.m_x), torch.uint8, "synd_x"),
                self._chk(synd_z, (B, self.m_z), torch.uint8, "synd_z"))

    def _residual_in(self, ex, ez, x_hat, z_hat):
        """(B, ex, ez, x_hat, z_hat): the noise and its estimate, four uint8 [B, n]."""
        B = int(ex.shape[0])
        return (B, self._chk(ex, (B, self.n), torch.uint8, "noise_x"), self._chk(ez, (B, self.n), torch.uint8, "noise_z"),
                self._chk(x_hat, (B, self.n), torch.uint8, "x_hat"), self._chk(z_hat, (B, self.n), torch.uint8, "z_hat"))

    def _gamma_in(self, gamma):
        """Memory strengths [num_legs, n] float32."""
        if gamma.dim() != 2 or gamma.shape[0] < 1:
            raise ValueError("gamma must have shape [num_legs, n]")
        return self._chk(gamma, (int(gamma.shape[0]), self.n), torch.float32, "gamma")

    @staticmethod
    def _tables_in(factors, owns):
        """The per-attempt host tables of `mbp4_decode` / `dsbp4_decode` as flat float32 arrays of one length."""
        factors = np.ascontiguousarray(np.asarray(factors, dtype=np.float32).reshape(-1))
        owns = np.ascontiguousarray(np.asarray(owns, dtype=np.float32).reshape(-1))
        if len(factors) != len(owns):
            raise ValueError("factors and owns must have the same length")
        return factors, owns

    def _osd_in(self, side, synd, e_hat, marg, llr_bin, index, chosen=None):
        """(B, synd, e_hat, marg, llr_bin, index, chosen) of the OSD calls; all but the first two may be None."""
        B = int(synd.shape[0])
        synd = self._chk(synd, (B, self.m_x if side == 0 else self.m_z), torch.uint8, "synd")
        e_hat = self._chk_out(e_hat, (B, self.n), torch.uint8, "e_hat")
        marg = self._opt_any(marg, torch.float32, "marg")
        llr_bin = self._opt_any(llr_bin, torch.float32, "llr_bin")
        index = self._opt_any(index, torch.int32, "index")
        if chosen is not None:
            chosen = self._chk_out(chosen, (B,), torch.int32, "chosen")
        return B, synd, e_hat, marg, llr_bin, index, chosen

    def _chk_counter(self, t, shape, name):
        """A device counter array the library adds to in place: contiguous int64 (or uint64) of ``shape``."""
        if t.device != self.device or t.dtype not in (torch.int64, torch.uint64) or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous int64{list(shape)} on {self.device}")

    def _new_xzs(self, B):
        """The outputs of a step-loop decoder: x_hat, z_hat [B, n] uint8 and stats [B, 4] int32."""
        return self._new((B, self.n), torch.uint8), self._new((B, self.n), torch.uint8), self._new((B, 4), torch.int32)

    def _noise_out(self, B, out):
        """(ex, ez) [B, n] uint8 of a noise call: new ones, or the caller's ``out=(ex, ez)`` checked as in-place buffers."""
        if out is None:
            return self._new((B, self.n), torch.uint8), self._new((B, self.n), torch.uint8)
        return self._chk_out(out[0], (B, self.n), torch.uint8, "noise_x"), self._chk_out(out[1], (B, self.n), torch.uint8, "noise_z")

    # ---- QLDPCBPDecoder.call ---------------------------------------------------------------------
    def _bp4_in(self, synd_x, synd_z, llr_ch, msg_init):
        """(B, synd_x, synd_z, llr_ch, msg_init_x, msg_init_z) of `bp4_decode`, `bp4_decode_layered` and `bp4_decode_trace`."""
        B = int(synd_x.shape[0])
        synd_x = self._chk(synd_x, (B, self.m_x), torch.uint8, "synd_x")
        synd_z = self._chk(synd_z, (B, self.m_z), torch.uint8, "synd_z")
        if llr_ch is not None:
            llr_ch = self._chk(llr_ch, (B, 3, self.n), torch.float32, "llr_ch")
        mix = miz = None
        if msg_init is not None:
            mix = self._chk(msg_init[0], (B, self.E_x), torch.float32, "msg_init_x")
            miz = self._chk(msg_init[1], (B, self.E_z), torch.float32, "msg_init_z")
        return B, synd_x, synd_z, llr_ch, mix, miz

    def _bp4_run(self, fn, synd_x, synd_z, num_iter, cn_type, factor, llr_ch, llr_const, msg_init, return_msgs, want_logits):
        """The body of `bp4_decode` and `bp4_decode_layered`: ``fn`` is `fgnn_bp4_decode` or `fgnn_bp4_decode_layered` (one signature)."""
        cn = self._cn(cn_type)
        B, synd_x, synd_z, llr_ch, mix, miz = self._bp4_in(synd_x, synd_z, llr_ch, msg_init)
        llr = self._new((B, 3, self.n), torch.float32)
        xh = self._new((B, self.n), torch.uint8)
        zh = self._new((B, self.n), torch.uint8)
        xl = self._new((B, self.rows_xp), torch.float32) if want_logits else None
        zl = self._new((B, self.rows_zp), torch.float32) if want_logits else None
        mox = self._new((B, self.E_x), torch.float32) if return_msgs else None
        moz = self._new((B, self.E_z), torch.float32) if return_msgs else None
        check(fn(self.handle, cn, int(num_iter), float(factor), _ptr(llr_ch), float(llr_const), _ptr(synd_x), _ptr(synd_z), B, _ptr(mix),
                 _ptr(miz), _ptr(llr), _ptr(xh), _ptr(zh), _ptr(xl), _ptr(zl), _ptr(mox), _ptr(moz), _stream(self.device)))
        out = dict(llr=llr, x_hat=xh, z_hat=zh, x_logit=xl, z_logit=zl)
        if return_msgs:
            out["msg_x"], out["msg_z"] = mox, moz
        return out

    def bp4_decode(self, synd_x, synd_z, num_iter, cn_type="boxplus-phi", factor=1.0, llr_ch=None, llr_const=0.0,
                   msg_init=None, return_msgs=False, want_logits=True):
        return self._bp4_run(_lib.lib().fgnn_bp4_decode, synd_x, synd_z, num_iter, cn_type, factor, llr_ch, llr_const, msg_init,
                             return_msgs, want_logits)

    # ---- layered (serial) schedule ---------------------------------------------------------------
    def set_layers(self, layer_of=None):
        """Install the layering of `bp4_decode_layered` (fgnn_graph_set_layers): ``layer_of`` [m_x + m_z] gives every check (hx checks
        first, then hz) its layer 0 .. max; None installs the greedy layering.  No layer may be empty and no two checks of a layer may
        share a qubit, across hx and hz: a ValueError names the offender."""
        self._set_layering("fgnn_graph_set_layers", self.m_x + self.m_z, layer_of)

    def layers(self):
        """(num_layers, layer_of [m_x + m_z] int32) of the installed layering; (0, None) when there is none yet."""
        return self._get_layering("fgnn_graph_layers", self.m_x + self.m_z)

    def _set_layering(self, symbol, length, layer_of):
        """The three layerings (checks, bits, qubits) are installed alike: ``layer_of`` [length], or None for the greedy one."""
        install = getattr(_lib.lib(), symbol)
        if layer_of is None:
            check(install(self.handle, 0, None))
            return
        lay = np.ascontiguousarray(layer_of, dtype=np.int32)
        if lay.shape != (length,):
            raise ValueError(f"layer_of must have shape ({length},), got {lay.shape}")
        check(install(self.handle, int(lay.max()) + 1, _np_ptr(lay)))

    def _get_layering(self, symbol, length):
        read = getattr(_lib.lib(), symbol)
        num = C.c_int32(0)
        check(read(self.handle, C.byref(num), None))
        if num.value == 0:
            return 0, None
        lay = np.empty(length, np.int32)
        check(read(self.handle, C.byref(num), _np_ptr(lay)))
        return int(num.value), lay

    def bp4_decode_layered(self, synd_x, synd_z, num_iter, cn_type="boxplus-phi", factor=1.0, llr_ch=None, llr_const=0.0,
                           msg_init=None, return_msgs=False, want_logits=True):
        """`bp4_decode` in the layered (serial) schedule (fgnn_bp4_decode_layered): the checks are updated layer by layer, every update
        sees the results of the layers before it.  Same keywords and the same result dict; a graph without a layering gets the greedy
        one (`set_layers`)."""
        return self._bp4_run(_lib.lib().fgnn_bp4_decode_layered, synd_x, synd_z, num_iter, cn_type, factor, llr_ch, llr_const, msg_init,
                             return_msgs, want_logits)

    def bp4_decode_trace(self, synd_x, synd_z, num_iter, cn_type="boxplus-phi", factor=1.0, llr_ch=None, llr_const=0.0,
                         msg_init=None, want_tape=False):
        """One launch of `num_iter` iterations that records the soft syndromes after 0, 1, ..., num_iter iterations
        (fgnn_bp4_decode_trace: the reference's trainable / stage_two return mode, decoding_q.py:743-746).  Returns
        dict(llr, x_hat, z_hat, x_logit [T+1,B,rows0], z_logit [T+1,B,rows1]) and, with ``want_tape``, tape_x [T+1,B,E_x] /
        tape_z [T+1,B,E_z] (the c->v messages before every iteration, the last slot after the last one)."""
        cn, T = self._cn(cn_type), int(num_iter)
        B, synd_x, synd_z, llr_ch, mix, miz = self._bp4_in(synd_x, synd_z, llr_ch, msg_init)
        llr = self._new((B, 3, self.n), torch.float32)
        xh = self._new((B, self.n), torch.uint8)
        zh = self._new((B, self.n), torch.uint8)
        xl = self._new((T + 1, B, self.rows_xp), torch.float32)
        zl = self._new((T + 1, B, self.rows_zp), torch.float32)
        tx = self._new((T + 1, B, self.E_x), torch.float32) if want_tape else None
        tz = self._new((T + 1, B, self.E_z), torch.float32) if want_tape else None
        check(_lib.lib().fgnn_bp4_decode_trace(self.handle, cn, T, float(factor), _ptr(llr_ch), float(llr_const),
                                               _ptr(synd_x), _ptr(synd_z), B, _ptr(mix), _ptr(miz), _ptr(llr), _ptr(xh), _ptr(zh),
                                               _ptr(xl), _ptr(zl), _ptr(tx), _ptr(tz), _stream(self.device)))
        out = dict(llr=llr, x_hat=xh, z_hat=zh, x_logit=xl, z_logit=zl)
        if want_tape:
            out["tape_x"], out["tape_z"] = tx, tz
        return out

    # ---- Feedback_GNN.call -------------------------------------------------------------------------
    def feedback_gnn(self, weights, llr, logit_hx, logit_hz, synd_x, synd_z):
        B, llr, logit_hx, logit_hz, synd_x, synd_z = self._gnn_in(llr, logit_hx, logit_hz, synd_x, synd_z)
        out = self._new((B, 3, self.n), torch.float32)
        check(_lib.lib().fgnn_feedback_gnn(self.handle, weights.handle, _ptr(llr), _ptr(logit_hx), _ptr(logit_hz),
                                           _ptr(synd_x), _ptr(synd_z), B, _ptr(out), _stream(self.device)))
        return out

    # ---- reverse pass of the second training stage (Second_Stage_GNN_BP_Model + tf.GradientTape) ----------
    def bp4_logit_trace(self, llr_ch, synd_x, synd_z, num_iter, factor=1.0, chained=False):
        """Forward of the stage_two decoder with a tape (``chained``: as T chained one-iteration launches, the round-1/2 form kept
        as the cross-check of the one-launch kernel).  Returns
        dict(tape_x [T+1,B,E_x], tape_z [T+1,B,E_z], x_logit [T+1,B,rows0], z_logit [T+1,B,rows1], x_hat, z_hat, llr)."""
        if not chained:  # one launch: the kernel records the soft syndromes and the tape itself (fgnn_bp4_decode_trace)
            return self.bp4_decode_trace(synd_x, synd_z, num_iter, "boxplus-phi", factor, llr_ch=llr_ch, want_tape=True)
        B, T = int(llr_ch.shape[0]), int(num_iter)
        tx = self._new((T + 1, B, self.E_x), torch.float32).zero_()
        tz = self._new((T + 1, B, self.E_z), torch.float32).zero_()
        xl = self._new((T + 1, B, self.rows_xp), torch.float32)
        zl = self._new((T + 1, B, self.rows_zp), torch.float32)
        out = self.bp4_decode(synd_x, synd_z, 0, "boxplus-phi", factor, llr_ch=llr_ch)
        xl[0], zl[0] = out["x_logit"], out["z_logit"]
        for k in range(T):
            out = self.bp4_decode(synd_x, synd_z, 1, "boxplus-phi", factor, llr_ch=llr_ch, msg_init=(tx[k], tz[k]),
                                  return_msgs=True)
            tx[k + 1], tz[k + 1] = out["msg_x"], out["msg_z"]
            xl[k + 1], zl[k + 1] = out["x_logit"], out["z_logit"]
        return dict(tape_x=tx, tape_z=tz, x_logit=xl, z_logit=zl, x_hat=out["x_hat"], z_hat=out["z_hat"], llr=out["llr"])

    def bp4_backward(self, llr_ch, synd_x, synd_z, tape_x, tape_z, grad_x_logit, grad_z_logit, factor=1.0):
        """d loss / d llr_ch [B,3,n] from d loss / d soft syndromes [T+1,B,rows] (fgnn_bp4_backward); a side whose gradient is None
        contributes nothing (the library's NULL)."""
        T, B = int(tape_x.shape[0]) - 1, int(llr_ch.shape[0])
        llr_ch = self._chk(llr_ch, (B, 3, self.n), torch.float32, "llr_ch")
        synd_x = self._chk(synd_x, (B, self.m_x), torch.uint8, "synd_x")
        synd_z = self._chk(synd_z, (B, self.m_z), torch.uint8, "synd_z")
        tape_x = self._chk(tape_x, (T + 1, B, self.E_x), torch.float32, "tape_x")
        tape_z = self._chk(tape_z, (T + 1, B, self.E_z), torch.float32, "tape_z")
        gx = self._opt(grad_x_logit, (T + 1, B, self.rows_xp), torch.float32, "grad_x_logit")
        gz = self._opt(grad_z_logit, (T + 1, B, self.rows_zp), torch.float32, "grad_z_logit")
        flags = [(t != 0).flatten(1).any(1) for t in (gx, gz) if t is not None]
        if flags:
            has = (flags[0] | flags[-1]).to(torch.uint8).contiguous()
        else:
            has = self._new((T + 1,), torch.uint8).zero_()
        out = self._new((B, 3, self.n), torch.float32)
        check(_lib.lib().fgnn_bp4_backward(self.handle, T, float(factor), _ptr(llr_ch), _ptr(synd_x), _ptr(synd_z), B,
                                           _ptr(tape_x), _ptr(tape_z), _ptr(gx), _ptr(gz), _ptr(has), _ptr(out),
                                           _stream(self.device)))
        return out

    def feedback_gnn_backward_pairs(self, weights, llr, logit_hx, logit_hz, synd_x, synd_z, grad_out):
        """The reverse kernels' own outputs: one (input activations [rows, K], pre-activation deltas [rows, J]) pair per Dense layer
        in execution order — hx message MLP, hz message MLP (rows = B * E_s, the edges in the order of `edges(s)`), embed MLP,
        _llr_inv_embed (rows = B * n).  The one place their buffers are sized and handed to the library.  Shipped configuration
        (fgnn_feedback_gnn_backward): (e_feat, e_d1), (e_h1, e_dm) per side, (node_in, node_d2) with node_in 44 wide (column 43 is
        padding), (node_h2, grad_out as rows); any other (fgnn_feedback_gnn_backward_general): acts[li], deltas[li]."""
        B, llr, logit_hx, logit_hz, synd_x, synd_z = self._gnn_in(llr, logit_hx, logit_hz, synd_x, synd_z)
        grad_out = self._chk(grad_out, (B, 3, self.n), torch.float32, "grad_out")
        if weights.general:
            D, H, L, _, _, _ = weights.config
            shapes = [(4 if l == 0 else H, D if l == L - 1 else H) for _ in range(2) for l in range(L)]
            shapes += [(2 * D + 3 if l == 0 else H, H) for l in range(L - 1)]
            shapes += [(H if L > 1 else 2 * D + 3, 3)]
            rows = [B * self.E_x] * L + [B * self.E_z] * L + [B * self.n] * L
            acts = [self._new((r, k), torch.float32) for r, (k, _) in zip(rows, shapes)]
            deltas = [self._new((r, j), torch.float32) for r, (_, j) in zip(rows, shapes)]
            pa = (C.c_void_p * len(acts))(*[t.data_ptr() for t in acts])
            pd = (C.c_void_p * len(deltas))(*[t.data_ptr() for t in deltas])
            check(_lib.lib().fgnn_feedback_gnn_backward_general(self.handle, weights.handle, _ptr(llr), _ptr(logit_hx), _ptr(logit_hz),
                                                                _ptr(synd_x), _ptr(synd_z), B, _ptr(grad_out), pa, pd, len(acts),
                                                                _stream(self.device)))
            return list(zip(acts, deltas))
        node_in = self._new((B * self.n, 44), torch.float32)
        node_h2 = self._new((B * self.n, 40), torch.float32)
        node_d2 = self._new((B * self.n, 40), torch.float32)
        Es = (self.E_x, self.E_z)
        feat = [self._new((B * e, 4), torch.float32) for e in Es]
        h1 = [self._new((B * e, 40), torch.float32) for e in Es]
        d1 = [self._new((B * e, 40), torch.float32) for e in Es]
        dm = [self._new((B * e, 20), torch.float32) for e in Es]
        pp = lambda ts: (C.c_void_p * 2)(*[t.data_ptr() for t in ts])  # noqa: E731
        check(_lib.lib().fgnn_feedback_gnn_backward(self.handle, weights.handle, _ptr(llr), _ptr(logit_hx), _ptr(logit_hz),
                                                    _ptr(synd_x), _ptr(synd_z), B, _ptr(grad_out), _ptr(node_in),
                                                    _ptr(node_h2), _ptr(node_d2), pp(feat), pp(h1), pp(d1), pp(dm),
                                                    _stream(self.device)))
        G = grad_out.permute(0, 2, 1).reshape(B * self.n, 3)
        return [(feat[0], d1[0]), (h1[0], dm[0]), (feat[1], d1[1]), (h1[1], dm[1]), (node_in, node_d2), (node_h2, G)]

    def feedback_gnn_backward(self, weights, llr, logit_hx, logit_hz, synd_x, synd_z, grad_out):
        """Weight gradients (Keras order, _llr_inv_embed first) of sum(grad_out * Feedback_GNN(...)): the HIP kernel leaves the
        (activation, delta) pairs of the Dense layers in HBM (`feedback_gnn_backward_pairs`), the reductions over batch x edges are
        library GEMMs: kernel gradient = activations^T deltas, bias gradient = column sums of the deltas."""
        pairs = self.feedback_gnn_backward_pairs(weights, llr, logit_hx, logit_hz, synd_x, synd_z, grad_out)
        D, H, L, _, _, bias = weights.config
        kernels = gnn_weight_shapes(D, H, L, use_bias=False)
        grads = []
        for f in range(3 * L):
            a, d = pairs[3 * L - 1 if f == 0 else f - 1]  # get_weights() lists _llr_inv_embed first, the kernels run it last
            grads.append(a[:, :kernels[f][0]].t() @ d)  # (the slice drops node_in's padding column and nothing else)
            if bias:
                grads.append(d.sum(0))
        return grads

    # ---- channel / syndromes / flags / residual ---------------------------------------------------------
    def pauli_noise(self, seed, p, first_sample, B, out=None, first_dev=None):
        """``out=(ex, ez)``: write into the given contiguous uint8 [B, n] tensors (row slices of a larger batch).  ``first_dev`` (device
        int64 / uint64 [1]): the stream position is read on the device, sample b = ``first_dev[0] + first_sample + b``
        (fgnn_pauli_noise_dev: Monte-Carlo loops captured in a hipGraph)."""
        ex, ez = self._noise_out(B, out)
        with torch.cuda.device(self.device):  # graph-less entry points run on the current device
            if first_dev is None:
                check(_lib.lib().fgnn_pauli_noise(int(seed), float(np.float32(p)), int(first_sample), B, self.n, _ptr(ex), _ptr(ez),
                                                  _stream(self.device)))
            else:
                if first_dev.device != self.device or first_dev.dtype not in (torch.int64, torch.uint64) or first_dev.numel() != 1:
                    raise ValueError(f"first_dev must be one int64 on {self.device}")
                check(_lib.lib().fgnn_pauli_noise_dev(int(seed), float(np.float32(p)), _ptr(first_dev), int(first_sample), B, self.n,
                                                      _ptr(ex), _ptr(ez), _stream(self.device)))
        return ex, ez

    def pauli_noise_xyz(self, seed, px, py, pz, first_sample, B, out=None):
        """Pauli.call for any triple (px, py, pz), pauli.py:98-108 (fgnn_pauli_noise_xyz): the same Philox uniforms as `pauli_noise`."""
        ex, ez = self._noise_out(B, out)
        with torch.cuda.device(self.device):
            check(_lib.lib().fgnn_pauli_noise_xyz(int(seed), float(np.float32(px)), float(np.float32(py)), float(np.float32(pz)),
                                                  int(first_sample), B, self.n, _ptr(ex), _ptr(ez), _stream(self.device)))
        return ex, ez

    def pauli_noise_wt(self, seed, wt, first_sample, B, out=None):
        ex, ez = self._noise_out(B, out)
        with torch.cuda.device(self.device):
            check(_lib.lib().fgnn_pauli_noise_wt(int(seed), int(wt), int(first_sample), B, self.n, _ptr(ex), _ptr(ez),
                                                 _stream(self.device)))
        return ex, ez

    def syndrome(self, ex, ez):
        B = int(ex.shape[0])
        ex = self._chk(ex, (B, self.n), torch.uint8, "noise_x")
        ez = self._chk(ez, (B, self.n), torch.uint8, "noise_z")
        sx = self._new((B, self.m_x), torch.uint8)
        sz = self._new((B, self.m_z), torch.uint8)
        check(_lib.lib().fgnn_syndrome(self.handle, _ptr(ex), _ptr(ez), B, _ptr(sx), _ptr(sz), _stream(self.device)))
        return sx, sz

    def flag_update(self, x_hat, z_hat, synd_x, synd_z, errors):
        B = int(x_hat.shape[0])
        x_hat = self._chk(x_hat, (B, self.n), torch.uint8, "x_hat")
        z_hat = self._chk(z_hat, (B, self.n), torch.uint8, "z_hat")
        synd_x = self._chk(synd_x, (B, self.m_x), torch.uint8, "synd_x")
        synd_z = self._chk(synd_z, (B, self.m_z), torch.uint8, "synd_z")
        errors = self._chk_out(errors, (B,), torch.uint8, "errors")
        check(_lib.lib().fgnn_flag_update(self.handle, _ptr(x_hat), _ptr(z_hat), _ptr(synd_x), _ptr(synd_z), B, _ptr(errors),
                                          _stream(self.device)))
        return errors

    def merge(self, errors, x_upd, z_upd, x_hat, z_hat):
        B = int(x_hat.shape[0])
        errors = self._chk(errors, (B,), torch.uint8, "errors")
        x_upd = self._chk(x_upd, (B, self.n), torch.uint8, "x_upd")
        z_upd = self._chk(z_upd, (B, self.n), torch.uint8, "z_upd")
        x_hat = self._chk_out(x_hat, (B, self.n), torch.uint8, "x_hat")
        z_hat = self._chk_out(z_hat, (B, self.n), torch.uint8, "z_hat")
        with torch.cuda.device(self.device):  # fgnn_merge takes no graph: it runs on the current device
            check(_lib.lib().fgnn_merge(_ptr(errors), _ptr(x_upd), _ptr(z_upd), B, self.n, _ptr(x_hat), _ptr(z_hat),
                                        _stream(self.device)))

    def residual(self, ex, ez, x_hat, z_hat, want_arrays=True):
        B, ex, ez, x_hat, z_hat = self._residual_in(ex, ez, x_hat, z_hat)
        s_hat = self._new((B, self.m_z + self.m_x), torch.uint8) if want_arrays else None
        ls_hat = self._new((B, self.rows_hxp + self.rows_hzp), torch.uint8) if want_arrays else None
        flags = self._new((B,), torch.uint8)
        check(_lib.lib().fgnn_residual(self.handle, _ptr(ex), _ptr(ez), _ptr(x_hat), _ptr(z_hat), B, _ptr(s_hat), _ptr(ls_hat),
                                       _ptr(flags), _stream(self.device)))
        return s_hat, ls_hat, flags

    def count_flags(self, flags, counts):
        """counts (uint64/int64 [3] on device) += (#flagged, #block errors, #samples)."""
        flags = self._chk(flags, (int(flags.shape[0]),), torch.uint8, "flags")
        self._chk_counter(counts, (3,), "counts")
        with torch.cuda.device(self.device):  # fgnn_count_flags takes no graph: it runs on the current device
            check(_lib.lib().fgnn_count_flags(_ptr(flags), int(flags.shape[0]), _ptr(counts), _stream(self.device)))
        return counts

    def count_flags_batches(self, flags, batch, counts, ring):
        """``flags`` holds ``k = len(flags) // batch`` consecutive batches decoded as one launch: ``ring[j]`` (int64 [k, 3] rows of a
        device ring) = the counters after batch j, ``counts`` = the last row (fgnn_count_flags_batches)."""
        B, batch = int(flags.shape[0]), int(batch)
        if batch <= 0 or B % batch:
            raise ValueError("flags must hold a whole number of batches")
        k = B // batch
        flags = self._chk(flags, (B,), torch.uint8, "flags")
        self._chk_counter(counts, (3,), "counts")
        self._chk_counter(ring, (k, 3), "ring")
        scratch = self._new((2 * k,), torch.int32)
        with torch.cuda.device(self.device):
            check(_lib.lib().fgnn_count_flags_batches(_ptr(flags), k, batch, _ptr(counts), _ptr(ring), _ptr(scratch),
                                                      _stream(self.device)))
        return counts

    # ---- Sandwich body -----------------------------------------------------------------------------------
    def sandwich_workspace(self, B):
        nbytes = _lib.lib().fgnn_sandwich_workspace_bytes(self.handle, int(B))
        return self._new((nbytes,), torch.uint8)

    def sandwich_decode(self, synd_x, synd_z, iters, weights_list, llr_const, factors=None, cn_types=None, compact=False,
                        workspace=None, return_llr=False, return_rounds=False):
        """fgnn_sandwich_decode.  ``compact=True`` runs each feedback round only on the samples still flagged: ``x_hat`` /
        ``z_hat`` / ``rounds`` are identical to the full run, but ``llr`` (``return_llr``) of a sample that left the flagged
        set holds the marginals of the LAST decoder that ran on it, where the full run holds those of the last decoder of the
        stack (which the reference computes for every sample and then ignores, feedback_gnn.py:336-340)."""
        num_layers = len(iters)
        if len(weights_list) != num_layers - 1:
            raise ValueError("need num_layers-1 feedback GNNs")
        if not self.stage_one:
            raise ValueError("the sandwich needs a stage_one graph")
        factors = [1.0] * num_layers if factors is None else list(factors)
        cn_types = ["boxplus-phi"] * num_layers if cn_types is None else list(cn_types)
        it = np.asarray(iters, dtype=np.int32)
        fa = np.asarray(factors, dtype=np.float32)
        ct = np.asarray([CN_TYPES[c] for c in cn_types], dtype=np.int32)
        wh = (C.c_void_p * max(1, num_layers - 1))(*[w.handle for w in weights_list])
        B, synd_x, synd_z = self._syndromes_in(synd_x, synd_z)
        if workspace is None:
            workspace = self.sandwich_workspace(B)
        xh = self._new((B, self.n), torch.uint8)
        zh = self._new((B, self.n), torch.uint8)
        llr = self._new((B, 3, self.n), torch.float32) if return_llr else None
        rounds = self._new((B,), torch.uint8) if return_rounds else None
        check(_lib.lib().fgnn_sandwich_decode(self.handle, num_layers, _np_ptr(it), _np_ptr(fa), _np_ptr(ct), wh,
                                              float(llr_const), _ptr(synd_x), _ptr(synd_z), B, int(bool(compact)), _ptr(xh),
                                              _ptr(zh), _ptr(llr), _ptr(rounds), _ptr(workspace), workspace.numel(),
                                              _stream(self.device)))
        out = dict(x_hat=xh, z_hat=zh)
        if return_llr:
            out["llr"] = llr
        if return_rounds:
            out["rounds"] = rounds
        return out

    def forms_agreement(self, synd_x, synd_z, iters, weights_list, llr_const, chunk=16384, factors=None, cn_types=None):
        """The sandwich on the same syndromes under the two OPT-IN re-associations (options 4 and 5 = 1) and under the library's default,
        the reference's formulas term by term (options 4 and 5 = 0: one Dense per edge, feedback_gnn.py:175-184; one log-sum-exp per
        edge, decoding_q.py:254-273), compared per sample: how many samples end on different decisions, how far the marginals of the
        last decoder (and of the first decoder alone) are apart — over all samples and over the samples both forms solve (a sample
        BP does not converge on is chaotic under ANY change of float32 rounding).  Both runs are this library's
        kernels, each bit-equal to the oracle's restatement of its form; the settings in force are restored."""
        B = int(synd_x.shape[0])
        factors = [1.0] * len(iters) if factors is None else list(factors)
        cn_types = ["boxplus-phi"] * len(iters) if cn_types is None else list(cn_types)
        prev = (self.gnn_factored, self.bp4_shared_lse)
        res = dict(samples=B, decisions_differ=0, max_abs_dllr=0.0, samples_gt_1e_4=0, max_abs_dllr_solved=0.0,
                   samples_gt_1e_4_solved=0, flagged_reassociated=0, flagged_literal=0, flagged_in_one_form_only=0,
                   first_decoder=dict(decisions_differ=0, max_abs_dllr=0.0, samples_gt_1e_4=0))
        try:
            for s in range(0, B, chunk):
                sx, sz = synd_x[s:s + chunk].contiguous(), synd_z[s:s + chunk].contiguous()
                outs = []
                for reassociated in (True, False):
                    self.set_gnn_factored(reassociated)
                    self.set_bp4_shared_lse(reassociated)
                    o = self.sandwich_decode(sx, sz, iters, weights_list, llr_const, factors=factors, cn_types=cn_types, return_llr=True)
                    o["flag"] = self.flag_update(o["x_hat"], o["z_hat"], sx, sz, self._new((sx.shape[0],), torch.uint8).fill_(1)) != 0
                    o["first"] = self.bp4_decode(sx, sz, iters[0], cn_types[0], factors[0], llr_const=llr_const, want_logits=False)
                    outs.append(o)
                a, b = outs
                differ = (a["x_hat"] != b["x_hat"]).any(1) | (a["z_hat"] != b["z_hat"]).any(1)
                d = (a["llr"] - b["llr"]).abs().flatten(1).max(1).values
                solved = ~(a["flag"] | b["flag"])
                res["decisions_differ"] += int(differ.sum())
                res["max_abs_dllr"] = max(res["max_abs_dllr"], float(d.max()))
                res["samples_gt_1e_4"] += int((d > 1e-4).sum())
                if bool(solved.any()):
                    res["max_abs_dllr_solved"] = max(res["max_abs_dllr_solved"], float(d[solved].max()))
                res["samples_gt_1e_4_solved"] += int((d[solved] > 1e-4).sum())
                res["flagged_reassociated"] += int(a["flag"].sum())
                res["flagged_literal"] += int(b["flag"].sum())
                res["flagged_in_one_form_only"] += int((a["flag"] ^ b["flag"]).sum())
                fa, fb, f = a["first"], b["first"], res["first_decoder"]
                d1 = (fa["llr"] - fb["llr"]).abs().flatten(1).max(1).values
                f["decisions_differ"] += int(((fa["x_hat"] != fb["x_hat"]).any(1) | (fa["z_hat"] != fb["z_hat"]).any(1)).sum())
                f["max_abs_dllr"] = max(f["max_abs_dllr"], float(d1.max()))
                f["samples_gt_1e_4"] += int((d1 > 1e-4).sum())
        finally:
            self.set_gnn_factored(prev[0])
            self.set_bp4_shared_lse(prev[1])
        return res

    # ---- OSD-0 (bp_osd.py) -----------------------------------------------------------------------------------------
    def set_basis(self, side, pivot_rows):
        piv = np.ascontiguousarray(pivot_rows, dtype=np.int32)
        check(_lib.lib().fgnn_graph_set_basis(self.handle, int(side), len(piv), _np_ptr(piv)))

    def compact(self, mask, bit=1):
        """Device index list of the samples with (mask & bit) != 0 and their count (one 4-byte device->host read)."""
        B = int(mask.shape[0])
        mask = self._chk(mask, (B,), torch.uint8, "mask")
        index = self._new((max(B, 1),), torch.int32)
        count = self._new((1,), torch.int32).zero_()
        with torch.cuda.device(self.device):
            check(_lib.lib().fgnn_compact(_ptr(mask), int(bit), B, _ptr(index), _ptr(count), _stream(self.device)))
        return index, int(count.item())

    def osd0(self, side, synd, e_hat, marg=None, llr_bin=None, index=None, nact=0):
        """Overwrite e_hat[b] (uint8 [B,n]) for the listed samples with the OSD-0 solution of side 0 (hx) / 1 (hz)."""
        B, synd, e_hat, marg, llr_bin, index, _ = self._osd_in(side, synd, e_hat, marg, llr_bin, index)
        check(_lib.lib().fgnn_osd0(self.handle, int(side), _ptr(marg), _ptr(llr_bin), _ptr(synd), B, _ptr(index), int(nact),
                                   _ptr(e_hat), _stream(self.device)))
        return e_hat

    def osd(self, side, synd, e_hat, method, order, marg=None, llr_bin=None, index=None, nact=0, chosen=None):
        """Overwrite e_hat[b] for the listed samples with the OSD-E / OSD-CS solution of side 0 (hx) / 1 (hz) (`fgnn_osd`): `method` a
        name of `OSD_METHODS` or its FGNN_OSD_* id, `order` the search depth.  `chosen` (int32 [B], optional) receives the winning
        candidate index of every processed sample (0 = the OSD-0 solution)."""
        method = osd_method_id(method)
        B, synd, e_hat, marg, llr_bin, index, chosen = self._osd_in(side, synd, e_hat, marg, llr_bin, index, chosen)
        check(_lib.lib().fgnn_osd(self.handle, int(side), method, int(order), _ptr(marg), _ptr(llr_bin), _ptr(synd), B, _ptr(index),
                                  int(nact), _ptr(e_hat), _ptr(chosen), _stream(self.device)))
        return e_hat

    # ---- OSD beyond LDS (fgnn_osd_ws) ------------------------------------------------------------------------------
    # default slot count: slots x slot bytes within this cap, clamped to [1, 2 x CUs].  The elimination is bound by the latency of its
    # row steps, not by bytes (57 MB moved per [[6480,1296]] sample): more concurrent samples win over a cache-sized working set
    # (profiles/osd_large.json: 64 slots 195 ms, 128 or more 111 ms for 100 failures)
    OSD_WS_CACHE_BYTES = 1 << 30

    def osd_resident(self, side, method="osd0"):
        """True iff the LDS-resident kernels take this side's basis: `osd0` for method "osd0", `osd` for "osd_e" / "osd_cs"."""
        fits = C.c_int()
        check(_lib.lib().fgnn_osd_resident(self.handle, int(side), osd_method_id(method), C.byref(fits)))
        return bool(fits.value)

    def osd_slot_bytes(self, side, method="osd0", order=0):
        nbytes = C.c_size_t()
        check(_lib.lib().fgnn_osd_workspace_bytes(self.handle, int(side), osd_method_id(method), int(order), 1, C.byref(nbytes)))
        return int(nbytes.value)

    def osd_default_slots(self, side, method="osd0", order=0):
        """Slots whose slot bytes fit OSD_WS_CACHE_BYTES together, clamped to [1, 2 x CUs]."""
        cus = torch.cuda.get_device_properties(self.device).multi_processor_count
        return max(1, min(2 * cus, self.OSD_WS_CACHE_BYTES // self.osd_slot_bytes(side, method, order)))

    def osd_workspace(self, side, method="osd0", order=0, slots=None, out=None):
        """A uint8 device workspace for `osd_ws` with `slots` slots (None: `osd_default_slots`).  `out` (optional) is returned
        instead when it is at least that large."""
        if slots is None:
            slots = self.osd_default_slots(side, method, order)
        nbytes = C.c_size_t()
        check(_lib.lib().fgnn_osd_workspace_bytes(self.handle, int(side), osd_method_id(method), int(order), int(slots), C.byref(nbytes)))
        if out is not None and out.numel() >= nbytes.value:
            return out
        return self._new((int(nbytes.value),), torch.uint8)

    def osd_ws(self, side, synd, e_hat, method, order, marg=None, llr_bin=None, index=None, nact=0, chosen=None, workspace=None):
        """`osd` (method "osd0": `osd0`) on a device workspace (`fgnn_osd_ws`): any basis with n <= 16384, the same outputs bit for
        bit.  `workspace` (uint8, from `osd_workspace`) sets the slot count; None allocates one with the default slot count."""
        method = osd_method_id(method)
        B, synd, e_hat, marg, llr_bin, index, chosen = self._osd_in(side, synd, e_hat, marg, llr_bin, index, chosen)
        if workspace is None:
            workspace = self.osd_workspace(side, method, order)
        workspace = self._chk_out(workspace, (workspace.numel(),), torch.uint8, "workspace")
        check(_lib.lib().fgnn_osd_ws(self.handle, int(side), method, int(order), _ptr(marg), _ptr(llr_bin), _ptr(synd), B, _ptr(index),
                                     int(nact), _ptr(e_hat), _ptr(chosen), _ptr(workspace), workspace.numel(), _stream(self.device)))
        return e_hat

    # ---- cluster post-processing (fgnn_lsd) ------------------------------------------------------------------------
    def lsd_max_pivots(self, side):
        """The largest `max_pivots` `lsd` takes for side 0 (hx) / 1 (hz): min(m_side, n, what the LDS holds)."""
        cap = C.c_int()
        check(_lib.lib().fgnn_lsd_max_pivots(self.handle, int(side), C.byref(cap)))
        return int(cap.value)

    def lsd(self, side, synd, e_hat, marg=None, llr_bin=None, index=None, nact=0, max_pivots=0, max_rounds=0, stats=None):
        """Overwrite e_hat[b] (uint8 [B,n]) for the listed samples with the LSD-0 solution of side 0 (hx) / 1 (hz) on the full matrix
        (`fgnn_lsd`; no row basis).  `max_pivots` = 0: `lsd_max_pivots(side)`; `max_rounds` = 0: no limit.  Returns `(e_hat, stats)`,
        stats int32 [B,4] = (found, rounds, columns appended, pivots) of every processed sample (the rows of the others are left as
        they were: uninitialised when `stats` is not handed in)."""
        B, synd, e_hat, marg, llr_bin, index, _ = self._osd_in(side, synd, e_hat, marg, llr_bin, index)
        stats = self._new((B, 4), torch.int32) if stats is None else self._chk_out(stats, (B, 4), torch.int32, "stats")
        check(_lib.lib().fgnn_lsd(self.handle, int(side), _ptr(marg), _ptr(llr_bin), _ptr(synd), B, _ptr(index), int(nact),
                                  int(max_pivots), int(max_rounds), _ptr(e_hat), _ptr(stats), _stream(self.device)))
        return e_hat, stats

    def residual_rows(self, rows_x, rows_z, ex, ez, x_hat, z_hat):
        B, ex, ez, x_hat, z_hat = self._residual_in(ex, ez, x_hat, z_hat)
        ls_hat = self._new((B, self._row_count(rows_x) + self._row_count(rows_z)), torch.uint8)
        flags = self._new((B,), torch.uint8)
        check(_lib.lib().fgnn_residual_rows(self.handle, int(rows_x), int(rows_z), _ptr(ex), _ptr(ez), _ptr(x_hat), _ptr(z_hat), B, None,
                                            _ptr(ls_hat), _ptr(flags), _stream(self.device)))
        return ls_hat, flags

    def _row_count(self, which):
        return [self.rows_xp, self.rows_zp, self.rows_hxp, self.rows_hzp, self.rows_lx, self.rows_lz][which]

    # ---- binary syndrome BP on the hx graph (LDPCBPDecoder, is_syndrome=True) ----------------------------------
    def bp2_decode(self, synd, num_iter, cn_type="boxplus-phi", factor=1.0, llr_ch=None, llr_const=0.0, B=None, want_soft=True,
                   want_hard=True):
        cn = self._cn(cn_type)
        B, synd, llr_ch = self._binary_in(synd, llr_ch, B)
        soft = self._new((B, self.n), torch.float32) if want_soft else None
        hard = self._new((B, self.n), torch.uint8) if want_hard else None
        check(_lib.lib().fgnn_bp2_decode(self.handle, cn, int(num_iter), float(factor), _ptr(llr_ch), float(llr_const),
                                         _ptr(synd), B, _ptr(soft), _ptr(hard), _stream(self.device)))
        return soft, hard

    # ---- layered (serial) schedule of binary BP ------------------------------------------------------------------
    def set_bit_layers(self, layer_of=None):
        """Install the layering of `bp2_decode_layered` (fgnn_graph_set_bit_layers): ``layer_of`` [m_x] gives every hx check its layer
        0 .. max; None installs the greedy layering.  No layer may be empty and no two checks of a layer may share a bit: a ValueError
        names the offender, and the installed layering stays.  Independent of `set_layers`."""
        self._set_layering("fgnn_graph_set_bit_layers", self.m_x, layer_of)

    def bit_layers(self):
        """(num_layers, layer_of [m_x] int32) of the installed bit layering; (0, None) when there is none yet."""
        return self._get_layering("fgnn_graph_bit_layers", self.m_x)

    def bp2_decode_layered(self, synd, num_iter, cn_type="boxplus-phi", factor=1.0, llr_ch=None, llr_const=0.0, B=None, want_soft=True,
                           want_hard=True, stop=False, want_stats=False):
        """`bp2_decode` in the layered (serial) schedule (fgnn_bp2_decode_layered): the hx checks are updated layer by layer on running
        posteriors, every update sees the results of the layers before it.  ``stop``: a sample leaves after the first iteration whose
        decision reproduces its syndrome.  Returns `(soft, hard)`, or with ``want_stats`` `(soft, hard, stats)`, stats int32 [B,2] =
        (the decision reproduces the syndrome, iterations run).  A graph without a bit layering gets the greedy one
        (`set_bit_layers`)."""
        cn = self._cn(cn_type)
        B, synd, llr_ch = self._binary_in(synd, llr_ch, B)
        soft = self._new((B, self.n), torch.float32) if want_soft else None
        hard = self._new((B, self.n), torch.uint8) if want_hard else None
        stats = self._new((B, 2), torch.int32) if want_stats else None
        check(_lib.lib().fgnn_bp2_decode_layered(self.handle, cn, int(num_iter), float(factor), _ptr(llr_ch), float(llr_const),
                                                 _ptr(synd), B, int(bool(stop)), _ptr(soft), _ptr(hard), _ptr(stats),
                                                 _stream(self.device)))
        return (soft, hard, stats) if want_stats else (soft, hard)

    def relay_decode(self, synd, gamma, pre_iter, leg_iter, stop_nconv, factor=1.0, llr_ch=None, llr_const=0.0, B=None):
        """Relay-BP on the hx graph (`fgnn_relay_decode`): `gamma` [num_legs, n] float32 on the device, one row of memory strengths per
        leg.  Returns `(hard [B,n] uint8, stats [B,4] int32 = found, weight, leg, k)`."""
        B, synd, llr_ch = self._binary_in(synd, llr_ch, B)
        gamma = self._gamma_in(gamma)
        hard = self._new((B, self.n), torch.uint8)
        stats = self._new((B, 4), torch.int32)
        check(_lib.lib().fgnn_relay_decode(self.handle, float(factor), int(pre_iter), int(gamma.shape[0]), int(leg_iter), int(stop_nconv),
                                           _ptr(gamma), _ptr(llr_ch), float(llr_const), _ptr(synd), B, _ptr(hard), _ptr(stats),
                                           _stream(self.device)))
        return hard, stats

    def relay_decode_layered(self, synd, gamma, pre_iter, leg_iter, stop_nconv, factor=1.0, llr_ch=None, llr_const=0.0, B=None):
        """`relay_decode` with legs in the layered (serial) schedule (`fgnn_relay_decode_layered`): every iteration of a leg updates the
        hx checks layer by layer on running posteriors.  Arguments and return as `relay_decode`.  A graph without a bit layering gets
        the greedy one (`set_bit_layers`)."""
        B, synd, llr_ch = self._binary_in(synd, llr_ch, B)
        gamma = self._gamma_in(gamma)
        hard = self._new((B, self.n), torch.uint8)
        stats = self._new((B, 4), torch.int32)
        check(_lib.lib().fgnn_relay_decode_layered(self.handle, float(factor), int(pre_iter), int(gamma.shape[0]), int(leg_iter),
                                                   int(stop_nconv), _ptr(gamma), _ptr(llr_ch), float(llr_const), _ptr(synd), B, _ptr(hard),
                                                   _ptr(stats), _stream(self.device)))
        return hard, stats

    def gdg_workspace_bytes(self, depth, nact):
        """Bytes of device workspace `fgnn_gdg_decode` needs for `nact` samples at `depth`."""
        nbytes = C.c_size_t()
        check(_lib.lib().fgnn_gdg_workspace_bytes(self.handle, int(depth), int(nact), C.byref(nbytes)))
        return int(nbytes.value)

    def gdg_decode(self, synd, pre_iter, round_iter, max_rounds, depth, tail="least", decim_llr=25.0, factor=0.8, llr_ch=None,
                   llr_const=0.0, B=None, index=None, nact=None, want_path_stats=False, out=None):
        """BP-GDG on the hx graph (`fgnn_gdg_decode`): min-sum BP with guided decimation guessing, 2**depth paths per sample.  `tail`
        = "least" / "most": the bit the picks after the first `depth` take; `max_rounds` None = n.  `index` (int32 on the device) lists
        the samples to decode, `nact` how many of its entries count (None: all); the rows of the other samples are those of `out` =
        `(hard, stats)`, written in place, or zeros without it.  Returns `(hard [B,n] uint8, stats [B,4] int32 = paths that found a
        solution, weight, path, bits fixed)`, and with `want_path_stats` `path_stats [nact, 2**depth, 4]` int32 = (found, weight, bits
        fixed, iterations) per listed sample and path.  The workspace is allocated here, from `fgnn_gdg_workspace_bytes`."""
        if tail not in _lib.GDG_TAILS:
            raise ValueError('tail must be "least" or "most"')
        B, synd, llr_ch = self._binary_in(synd, llr_ch, B)
        if B is None:
            raise ValueError("without a syndrome and llr_ch, B must be given")
        max_rounds = self.n if max_rounds is None else int(max_rounds)
        if index is not None:
            index = self._opt_any(index, torch.int32, "index")
            nact = int(index.numel()) if nact is None else int(nact)
            if not 0 <= nact <= min(int(index.numel()), B):
                raise ValueError("nact must be in 0 .. min(len(index), B)")
        else:
            nact = B
        if out is not None:
            hard = self._chk_out(out[0], (B, self.n), torch.uint8, "hard")
            stats = self._chk_out(out[1], (B, 4), torch.int32, "stats")
        elif index is not None:
            hard, stats = self._new((B, self.n), torch.uint8).zero_(), self._new((B, 4), torch.int32).zero_()
        else:
            hard, stats = self._new((B, self.n), torch.uint8), self._new((B, 4), torch.int32)
        ws_bytes = self.gdg_workspace_bytes(depth, nact)
        ws = self._new((max(ws_bytes, 1),), torch.uint8)
        path_stats = self._new((nact, 1 << int(depth), 4), torch.int32) if want_path_stats else None
        if index is not None and index.numel() == 0:
            index = self._new((1,), torch.int32)  # an empty list still is a list: a NULL pointer would mean all B samples
        check(_lib.lib().fgnn_gdg_decode(self.handle, float(factor), int(pre_iter), int(round_iter), max_rounds, int(depth),
                                         _lib.GDG_TAILS[tail], float(decim_llr), _ptr(llr_ch), float(llr_const), _ptr(synd), B,
                                         _ptr(index), nact, _ptr(hard), _ptr(stats), _ptr(path_stats), _ptr(ws), ws_bytes,
                                         _stream(self.device)))
        return (hard, stats, path_stats) if want_path_stats else (hard, stats)

    def si_decode(self, synd, num_iter, si_iter, max_groups, factor=0.8, llr_ch=None, llr_const=0.0, B=None, index=None, nact=None,
                  out=None):
        """BP-SI on the hx graph (`fgnn_si_decode`): min-sum BP, then stabilizer inactivation with the rows of side 1 (hz) as the
        groups: up to `max_groups` of them, least reliable first, are erased one at a time, BP runs up to `si_iter` iterations on the
        rest and the erased bits come from a small linear system.  `index` (int32 on the device) lists the samples to decode, `nact`
        how many of its entries count (None: all); the rows of the other samples are those of `out` = `(hard, stats)`, written in
        place, or zeros without it.  Returns `(hard [B,n] uint8, stats [B,4] int32 = found, attempt, iteration within it, group or
        -1)`; a sample without a solution keeps plain BP's decision."""
        B, synd, llr_ch = self._binary_in(synd, llr_ch, B)
        if B is None:
            raise ValueError("without a syndrome and llr_ch, B must be given")
        if index is not None:
            index = self._opt_any(index, torch.int32, "index")
            nact = int(index.numel()) if nact is None else int(nact)
            if not 0 <= nact <= min(int(index.numel()), B):
                raise ValueError("nact must be in 0 .. min(len(index), B)")
        else:
            nact = B
        if out is not None:
            hard = self._chk_out(out[0], (B, self.n), torch.uint8, "hard")
            stats = self._chk_out(out[1], (B, 4), torch.int32, "stats")
        elif index is not None:
            hard, stats = self._new((B, self.n), torch.uint8).zero_(), self._new((B, 4), torch.int32).zero_()
        else:
            hard, stats = self._new((B, self.n), torch.uint8), self._new((B, 4), torch.int32)
        if index is not None and index.numel() == 0:
            index = self._new((1,), torch.int32)  # an empty list still is a list: a NULL pointer would mean all B samples
        check(_lib.lib().fgnn_si_decode(self.handle, float(factor), int(num_iter), int(si_iter), int(max_groups), _ptr(llr_ch),
                                        float(llr_const), _ptr(synd), B, _ptr(index), nact, _ptr(hard), _ptr(stats),
                                        _stream(self.device)))
        return hard, stats

    def relay4_decode(self, synd_x, synd_z, gamma, pre_iter, leg_iter, stop_nconv, factor=1.0, llr_ch=None, llr_const=0.0,
                      cn_type="minsum", B=None):
        """Relay-BP4 on both graphs (`fgnn_relay4_decode`): `gamma` [num_legs, n] float32 on the device, one row of memory strengths per
        leg; `llr_ch` [B, 3, n] or one `llr_const` for all three LLRs of every qubit; a syndrome that is None is all-zero.  Returns
        `(x_hat [B,n] uint8, z_hat [B,n] uint8, stats [B,4] int32 = found, weight, leg, k)`."""
        cn = self._cn(cn_type)
        B, synd_x, synd_z, llr_ch = self._quaternary_in(synd_x, synd_z, llr_ch, B)
        if gamma is not None:
            gamma = self._gamma_in(gamma)
        num_legs = int(gamma.shape[0]) if gamma is not None else 1
        xh, zh, stats = self._new_xzs(B)
        check(_lib.lib().fgnn_relay4_decode(self.handle, cn, float(factor), int(pre_iter), num_legs, int(leg_iter),
                                            int(stop_nconv), _ptr(gamma), _ptr(llr_ch), float(llr_const), _ptr(synd_x), _ptr(synd_z), B,
                                            _ptr(xh), _ptr(zh), _ptr(stats), _stream(self.device)))
        return xh, zh, stats

    def bp4gd_decode(self, synd_x, synd_z, pre_iter, round_iter, max_rounds=None, decim_llr=25.0, cn_type="minsum", factor=1.0,
                     llr_ch=None, llr_const=0.0, B=None):
        """BP4 with guided decimation on both graphs (`fgnn_bp4gd_decode`): up to `pre_iter` iterations, then up to `max_rounds` (None:
        n) rounds that fix the free qubit of largest margin to its decision (LLR magnitude `decim_llr`) and run up to `round_iter`
        iterations more; `llr_ch` [B, 3, n] or one `llr_const` for all three LLRs of every qubit; a syndrome that is None is all-zero.
        Returns `(x_hat [B,n] uint8, z_hat [B,n] uint8, stats [B,4] int32 = found, qubits fixed, iterations, k of the last test)`."""
        cn = self._cn(cn_type)
        B, synd_x, synd_z, llr_ch = self._quaternary_in(synd_x, synd_z, llr_ch, B)
        max_rounds = self.n if max_rounds is None else int(max_rounds)
        xh, zh, stats = self._new_xzs(B)
        check(_lib.lib().fgnn_bp4gd_decode(self.handle, cn, float(factor), int(pre_iter), int(round_iter), max_rounds,
                                           float(decim_llr), _ptr(llr_ch), float(llr_const), _ptr(synd_x), _ptr(synd_z), B, _ptr(xh),
                                           _ptr(zh), _ptr(stats), _stream(self.device)))
        return xh, zh, stats

    def bp4fb_decode(self, synd_x, synd_z, rule, pre_iter, attempt_iter, max_attempts, strength, cn_type="minsum", factor=1.0,
                     restart=False, seed=0x5EED, first_sample=0, llr_ch=None, llr_const=0.0, B=None):
        """BP4 with prior feedback on both graphs (`fgnn_bp4fb_decode`): up to `pre_iter` iterations, then up to `max_attempts` times
        the rule `"perturb"` or `"enhanced"` changes the channel LLRs (by `strength`) at qubits of the unsatisfied checks and BP4 runs
        up to `attempt_iter` iterations more, from the messages it has or, with `restart`, from zero messages.  The rules draw from the
        Philox stream of `seed` at the global sample indices `first_sample` .. `first_sample + B - 1`; `llr_ch` [B, 3, n] or one
        `llr_const` for all three LLRs of every qubit; a syndrome that is None is all-zero.  Returns `(x_hat [B,n] uint8, z_hat [B,n]
        uint8, stats [B,4] int32 = found, feedback steps made, iterations, k of the last test)`."""
        cn = self._cn(cn_type)
        if rule not in _lib.FB_RULES:
            raise ValueError('rule must be "perturb" or "enhanced"')
        B, synd_x, synd_z, llr_ch = self._quaternary_in(synd_x, synd_z, llr_ch, B)
        if not 0 <= int(seed) < 1 << 64 or not 0 <= int(first_sample) < 1 << 64:
            raise ValueError("seed and first_sample must fit 64 unsigned bits")
        xh, zh, stats = self._new_xzs(B)
        check(_lib.lib().fgnn_bp4fb_decode(self.handle, _lib.FB_RULES[rule], cn, float(factor), int(pre_iter),
                                           int(attempt_iter), int(max_attempts), float(strength), int(restart), int(seed),
                                           int(first_sample), _ptr(llr_ch), float(llr_const), _ptr(synd_x), _ptr(synd_z), B, _ptr(xh),
                                           _ptr(zh), _ptr(stats), _stream(self.device)))
        return xh, zh, stats

    def bp4aug_decode(self, synd_x, synd_z, pre_iter, attempt_iter, max_attempts, density, cn_type="minsum", factor=1.0, restart=True,
                      seed=0x5EED, first_sample=0, llr_ch=None, llr_const=0.0, B=None):
        """Augmented BP4 on both graphs (`fgnn_bp4aug_decode`): up to `pre_iter` iterations, then up to `max_attempts` times every
        check row is written a second time with probability `density` and BP4 runs up to `attempt_iter` iterations on that code, from
        zero messages with `restart`, else from the messages it has.  The marks are drawn from the Philox stream of `seed` at the
        global sample indices `first_sample` .. `first_sample + B - 1`; `llr_ch` [B, 3, n] or one `llr_const` for all three LLRs of
        every qubit; a syndrome that is None is all-zero.  Returns `(x_hat [B,n] uint8, z_hat [B,n] uint8, stats [B,4] int32 = found,
        draws made, iterations, k of the last test)`."""
        cn = self._cn(cn_type)
        B, synd_x, synd_z, llr_ch = self._quaternary_in(synd_x, synd_z, llr_ch, B)
        if not 0 <= int(seed) < 1 << 64 or not 0 <= int(first_sample) < 1 << 64:
            raise ValueError("seed and first_sample must fit 64 unsigned bits")
        xh, zh, stats = self._new_xzs(B)
        check(_lib.lib().fgnn_bp4aug_decode(self.handle, cn, float(factor), int(pre_iter), int(attempt_iter), int(max_attempts),
                                            float(density), int(restart), int(seed), int(first_sample), _ptr(llr_ch), float(llr_const),
                                            _ptr(synd_x), _ptr(synd_z), B, _ptr(xh), _ptr(zh), _ptr(stats), _stream(self.device)))
        return xh, zh, stats

    def mbp4_decode(self, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, llr_ch=None,
                    llr_const=0.0, B=None):
        """BP4 with message-strength control on both graphs (`fgnn_mbp4_decode`): attempt a (up to `pre_iter` iterations for a = 0,
        `attempt_iter` for the later ones) multiplies every check output by `factors[a]` and takes an edge's own message out of the
        qubit totals multiplied by `owns[a]`; the first estimate that reproduces both syndromes ends the codeword.  `factors` and
        `owns` are host sequences of the same length, 1 .. 64, rounded to float32 (Kuo-Lai's MBP4: owns[a] = alpha_a, factors[a] =
        base / alpha_a); with `restart` every attempt after the first starts from zero messages; `llr_ch` [B, 3, n] or one
        `llr_const` for all three LLRs of every qubit; a syndrome that is None is all-zero.  Returns `(x_hat [B,n] uint8, z_hat [B,n]
        uint8, stats [B,4] int32 = found, the attempt of the last test, iterations, k of the last test)`."""
        return self._mbp4_run(_lib.lib().fgnn_mbp4_decode, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type, restart, llr_ch,
                              llr_const, B)

    def _mbp4_run(self, fn, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type, restart, llr_ch, llr_const, B):
        """The body of `mbp4_decode` and `mbp4_decode_serial`: ``fn`` is `fgnn_mbp4_decode` or `fgnn_mbp4_decode_serial` (one
        signature)."""
        cn = self._cn(cn_type)
        factors, owns = self._tables_in(factors, owns)
        B, synd_x, synd_z, llr_ch = self._quaternary_in(synd_x, synd_z, llr_ch, B)
        xh, zh, stats = self._new_xzs(B)
        check(fn(self.handle, cn, len(factors), factors.ctypes.data, owns.ctypes.data, int(pre_iter), int(attempt_iter), int(restart),
                 _ptr(llr_ch), float(llr_const), _ptr(synd_x), _ptr(synd_z), B, _ptr(xh), _ptr(zh), _ptr(stats), _stream(self.device)))
        return xh, zh, stats

    # ---- serial schedule of MBP4: qubit by qubit -------------------------------------------------------------------
    def set_qubit_layers(self, layer_of=None):
        """Install the layering of `mbp4_decode_serial` (fgnn_graph_set_qubit_layers): ``layer_of`` [n] gives every qubit its layer
        0 .. max; None installs the greedy layering.  No layer may be empty and no two qubits of a layer may share a check, on hx or on
        hz: a ValueError names the offender, and the installed layering stays.  ``np.arange(n)`` is Kuo and Lai's literal order.
        Independent of `set_layers` and `set_bit_layers`."""
        self._set_layering("fgnn_graph_set_qubit_layers", self.n, layer_of)

    def qubit_layers(self):
        """(num_layers, layer_of [n] int32) of the installed qubit layering; (0, None) when there is none yet."""
        return self._get_layering("fgnn_graph_qubit_layers", self.n)

    def mbp4_decode_serial(self, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, llr_ch=None,
                           llr_const=0.0, B=None):
        """`mbp4_decode` in Kuo and Lai's serial schedule (fgnn_mbp4_decode_serial): the qubits are visited layer by layer, and a qubit
        sees the messages the qubits of the layers before it have just sent.  Same arguments and the same result; a graph without a
        qubit layering gets the greedy one (`set_qubit_layers`)."""
        return self._mbp4_run(_lib.lib().fgnn_mbp4_decode_serial, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type, restart,
                              llr_ch, llr_const, B)

    def dsbp4_decode(self, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, llr_ch=None,
                     llr_const=0.0, synd_llr_x=None, synd_llr_z=None, gamma_x=float("inf"), gamma_z=float("inf"), B=None):
        """Soft-syndrome BP4 on both graphs (`fgnn_dsbp4_decode`): `mbp4_decode` with a syndrome LLR per check and a joint stop test.
        `synd_llr_x` [B, m_x] / `synd_llr_z` [B, m_z] (float32) say how far each measured bit can be trusted; None means the scalar
        `gamma_x` / `gamma_z` for every check of that side (+inf, the default: a perfect measurement; NaN is refused).  The check rule
        takes the LLR as one more input, the decoder estimates which syndrome bits were wrong, and a sample is solved when the data
        estimate reproduces `synd ^ u_hat` on both graphs.  Every other argument is `mbp4_decode`'s.  Returns `(x_hat [B,n], z_hat
        [B,n], u_x_hat [B,m_x], u_z_hat [B,m_z]` uint8, `stats [B,4]` int32 = found, the attempt of the last test, iterations, k of the
        last test)`."""
        cn = self._cn(cn_type)
        factors, owns = self._tables_in(factors, owns)
        B, synd_x, synd_z, llr_ch = self._quaternary_in(synd_x, synd_z, llr_ch, B, also=(synd_llr_x, synd_llr_z),
                                                        missing="B is needed when neither syndromes nor llr_ch nor syndrome LLRs are given")
        synd_llr_x = self._opt(synd_llr_x, (B, self.m_x), torch.float32, "synd_llr_x")
        synd_llr_z = self._opt(synd_llr_z, (B, self.m_z), torch.float32, "synd_llr_z")
        xh = self._new((B, self.n), torch.uint8)
        zh = self._new((B, self.n), torch.uint8)
        uxh = self._new((B, self.m_x), torch.uint8)
        uzh = self._new((B, self.m_z), torch.uint8)
        stats = self._new((B, 4), torch.int32)
        check(_lib.lib().fgnn_dsbp4_decode(self.handle, cn, len(factors), factors.ctypes.data, owns.ctypes.data,
                                           int(pre_iter), int(attempt_iter), int(restart), _ptr(llr_ch), float(llr_const), _ptr(synd_x),
                                           _ptr(synd_z), _ptr(synd_llr_x), float(gamma_x), _ptr(synd_llr_z), float(gamma_z), B, _ptr(xh),
                                           _ptr(zh), _ptr(uxh), _ptr(uzh), _ptr(stats), _stream(self.device)))
        return xh, zh, uxh, uzh, stats

    def stbp4_decode(self, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, rounds=None,
                     prev_x=None, prev_z=None, llr_ch=None, llr_const=0.0, synd_llr_x=None, synd_llr_z=None, gamma_x=float("inf"),
                     gamma_z=float("inf"), gamma_last_x=float("inf"), gamma_last_z=float("inf"), B=None):
        """Space-time BP4 on a window of `rounds` repeated measurements (`fgnn_stbp4_decode`): `dsbp4_decode` on R copies of the two
        graphs, coupled by one time variable per check and round.  `synd_x` [B, R, m_x] / `synd_z` [B, R, m_z] (uint8) are the raw
        measured syndromes (None: all-zero), `prev_x` [B, m_x] / `prev_z` [B, m_z] the syndrome the window starts from (None: zero);
        the library forms the differences of consecutive rounds itself.  `llr_ch` [B, 3, n] or `llr_const` is the prior of a qubit in
        every round.  `gamma_x` / `gamma_z` are the syndrome LLRs of rounds 0 .. R-2 and `gamma_last_x` / `gamma_last_z` that of round
        R-1 (+inf, the default: a perfect read-out; NaN is refused); `synd_llr_x` [B, R, m_x] / `synd_llr_z` [B, R, m_z] (float32)
        replace both scalars of their side.  `rounds` = None takes R from the first of the syndromes and syndrome LLRs that is given.
        Every other argument is `mbp4_decode`'s.  Returns `(x_hat [B,R,n], z_hat [B,R,n]` = the error estimated for each round, not
        cumulative, `u_x_hat [B,R,m_x], u_z_hat [B,R,m_z]` uint8, `stats [B,4]` int32 = found, the attempt of the last test,
        iterations, k of the last test)`, per window.  A window that does not fit the LDS is refused with a ValueError that names the
        largest number of rounds that fits."""
        return self._stbp4_run(False, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type, restart, rounds, prev_x, prev_z, llr_ch,
                               llr_const, synd_llr_x, synd_llr_z, gamma_x, gamma_z, gamma_last_x, gamma_last_z, B)

    def stbp4_decode_soft(self, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type="minsum", restart=True, rounds=None,
                          prev_x=None, prev_z=None, llr_ch=None, llr_const=0.0, synd_llr_x=None, synd_llr_z=None, gamma_x=float("inf"),
                          gamma_z=float("inf"), gamma_last_x=float("inf"), gamma_last_z=float("inf"), B=None):
        """`stbp4_decode` with the soft values of the last test (`fgnn_stbp4_decode_soft`): the same arguments, and the same five
        outputs bit for bit, followed by `marg [B,R,3,n]`, `gam_x [B,R,m_x]` and `gam_z [B,R,m_z]` (float32).  For a window that was
        not solved they hold the totals X, Y, Z of every qubit and round and the Gamma of every time variable, the values the
        decisions and u_hat were taken from; the rows of a solved window are zero."""
        return self._stbp4_run(True, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type, restart, rounds, prev_x, prev_z, llr_ch,
                               llr_const, synd_llr_x, synd_llr_z, gamma_x, gamma_z, gamma_last_x, gamma_last_z, B)

    def _stbp4_run(self, soft, synd_x, synd_z, factors, owns, pre_iter, attempt_iter, cn_type, restart, rounds, prev_x, prev_z, llr_ch,
                   llr_const, synd_llr_x, synd_llr_z, gamma_x, gamma_z, gamma_last_x, gamma_last_z, B):
        """The checks, allocations and call of `stbp4_decode` and `stbp4_decode_soft`."""
        cn = self._cn(cn_type)
        factors, owns = self._tables_in(factors, owns)
        windows = (synd_x, synd_z, synd_llr_x, synd_llr_z)
        if rounds is None:
            rounds = next((int(t.shape[1]) for t in windows if t is not None and t.dim() == 3), None)
            if rounds is None:
                raise ValueError("rounds is needed when neither syndromes nor syndrome LLRs are given")
        R = int(rounds)
        if R < 1:
            raise ValueError("rounds must be >= 1")
        for t in (synd_x, synd_z, prev_x, prev_z, llr_ch, synd_llr_x, synd_llr_z):
            if t is not None:
                B = int(t.shape[0])
        if B is None:
            raise ValueError("B is needed when neither syndromes nor llr_ch nor syndrome LLRs are given")
        synd_x = self._opt(synd_x, (B, R, self.m_x), torch.uint8, "synd_x")
        synd_z = self._opt(synd_z, (B, R, self.m_z), torch.uint8, "synd_z")
        prev_x = self._opt(prev_x, (B, self.m_x), torch.uint8, "prev_x")
        prev_z = self._opt(prev_z, (B, self.m_z), torch.uint8, "prev_z")
        llr_ch = self._opt(llr_ch, (B, 3, self.n), torch.float32, "llr_ch")
        synd_llr_x = self._opt(synd_llr_x, (B, R, self.m_x), torch.float32, "synd_llr_x")
        synd_llr_z = self._opt(synd_llr_z, (B, R, self.m_z), torch.float32, "synd_llr_z")
        xh = self._new((B, R, self.n), torch.uint8)
        zh = self._new((B, R, self.n), torch.uint8)
        uxh = self._new((B, R, self.m_x), torch.uint8)
        uzh = self._new((B, R, self.m_z), torch.uint8)
        stats = self._new((B, 4), torch.int32)
        args = (self.handle, cn, len(factors), factors.ctypes.data, owns.ctypes.data, int(pre_iter), int(attempt_iter), int(restart), R,
                _ptr(llr_ch), float(llr_const), _ptr(synd_x), _ptr(synd_z), _ptr(prev_x), _ptr(prev_z), _ptr(synd_llr_x), float(gamma_x),
                float(gamma_last_x), _ptr(synd_llr_z), float(gamma_z), float(gamma_last_z), B, _ptr(xh), _ptr(zh), _ptr(uxh), _ptr(uzh),
                _ptr(stats))
        if not soft:
            check(_lib.lib().fgnn_stbp4_decode(*args, _stream(self.device)))
            return xh, zh, uxh, uzh, stats
        marg = self._new((B, R, 3, self.n), torch.float32)
        gam_x = self._new((B, R, self.m_x), torch.float32)
        gam_z = self._new((B, R, self.m_z), torch.float32)
        check(_lib.lib().fgnn_stbp4_decode_soft(*args, _ptr(marg), _ptr(gam_x), _ptr(gam_z), _stream(self.device)))
        return xh, zh, uxh, uzh, stats, marg, gam_x, gam_z

    # ---- one side of a window as a binary problem (fgnn_st_window_problem / fgnn_st_window_apply) -----------------------------------
    def _st_side(self, side):
        if side not in (0, 1):
            raise ValueError("side must be 0 or 1")
        return self.m_x if side == 0 else self.m_z

    def _st_index_in(self, index, nact):
        """(index, nact) of a window list: int32 on the device, at least `nact` entries (None: windows 0 .. nact-1)."""
        nact = int(nact)
        if nact < 0:
            raise ValueError("nact must be >= 0")
        if index is not None:
            index = self._opt_any(index, torch.int32, "index")
            if index.numel() < nact:
                raise ValueError(f"index holds {index.numel()} entries, nact is {nact}")
        return index, nact

    def st_window_problem(self, side, marg, gam, synd=None, prev=None, index=None, nact=None, rounds=None):
        """One side of the listed windows as the binary problem ``H_st [e ; u] = d`` (`fgnn_st_window_problem`): `marg [B,R,3,n]` and
        `gam [B,R,m_side]` are the soft outputs of `stbp4_decode_soft` for side 0 (hx: `gam_x`) or 1 (hz: `gam_z`), `synd [B,R,m_side]`
        / `prev [B,m_side]` the raw syndromes the decoder was given (None: zero).  `index` (int32, device) lists the windows and `nact`
        says how many of them count (`compact`); index None: windows 0 .. nact-1, nact None: all B.  Returns `(d [nact, R m_side]`
        uint8, `llr [nact, R (n + m_side)]` float32)`, row i for window index[i], in the row and column order of
        `space_time.window_matrix`: what `lsd` and `osd0` take as `synd` and `llr_bin` on that matrix's graph."""
        m = self._st_side(side)
        if marg.dim() != 4:
            raise ValueError("marg must have shape [B, R, 3, n]")
        B, R = int(marg.shape[0]), int(marg.shape[1]) if rounds is None else int(rounds)
        if R < 1:
            raise ValueError("rounds must be >= 1")
        marg = self._chk(marg, (B, R, 3, self.n), torch.float32, "marg")
        gam = self._chk(gam, (B, R, m), torch.float32, "gam")
        synd = self._opt(synd, (B, R, m), torch.uint8, "synd")
        prev = self._opt(prev, (B, m), torch.uint8, "prev")
        index, nact = self._st_index_in(index, B if nact is None else nact)
        if index is None and nact > B:
            raise ValueError(f"nact is {nact}, the batch holds {B} windows")
        d = self._new((nact, R * m), torch.uint8)
        llr = self._new((nact, R * (self.n + m)), torch.float32)
        check(_lib.lib().fgnn_st_window_problem(self.handle, int(side), R, _ptr(synd), _ptr(prev), _ptr(marg), _ptr(gam), _ptr(index), nact,
                                                _ptr(d), _ptr(llr), _stream(self.device)))
        return d, llr

    def st_window_apply(self, side, e, hat, u_hat, index=None, nact=None):
        """Write the solutions `e [nact, R (n + m_side)]` (uint8, the column order of `space_time.window_matrix`) of the listed
        windows into the decoder's outputs in place (`fgnn_st_window_apply`): side 0 takes `hat = z_hat [B,R,n]` and `u_hat = u_x_hat
        [B,R,m_x]`, side 1 `x_hat` and `u_z_hat`.  `index` / `nact` as `st_window_problem` (nact None: the rows of `e`); the rows of
        windows that are not listed are left as they are.  Returns `(hat, u_hat)`."""
        m = self._st_side(side)
        if hat.dim() != 3:
            raise ValueError("hat must have shape [B, R, n]")
        B, R = int(hat.shape[0]), int(hat.shape[1])
        hat = self._chk_out(hat, (B, R, self.n), torch.uint8, "hat")
        u_hat = self._chk_out(u_hat, (B, R, m), torch.uint8, "u_hat")
        index, nact = self._st_index_in(index, int(e.shape[0]) if nact is None else nact)
        if index is None and nact > B:
            raise ValueError(f"nact is {nact}, the batch holds {B} windows")
        if int(e.shape[0]) < nact:
            raise ValueError(f"e holds {int(e.shape[0])} rows, nact is {nact}")
        e = self._chk(e, (int(e.shape[0]), R * (self.n + m)), torch.uint8, "e")
        check(_lib.lib().fgnn_st_window_apply(self.handle, int(side), R, _ptr(e), _ptr(index), nact, _ptr(hat), _ptr(u_hat),
                                              _stream(self.device)))
        return hat, u_hat

    @staticmethod
    def syndrome_noise_seeds(seed):
        """The two stream seeds of `syndrome_noise`: ``(seed + 0x9E3779B97F4A7C15) mod 2^64`` for the hx checks and ``(seed + 2 *
        0x9E3779B97F4A7C15) mod 2^64`` for the hz checks."""
        step, mask = 0x9E3779B97F4A7C15, (1 << 64) - 1
        return (int(seed) + step) & mask, (int(seed) + 2 * step) & mask

    def syndrome_noise(self, seed, q, first_sample, B):
        """Measurement flips `(u_x [B, m_x], u_z [B, m_z])` uint8, each bit 1 with probability `q`: two calls of `fgnn_bsc_noise`, of
        width m_x on the seed ``(seed + 0x9E3779B97F4A7C15) mod 2^64`` and of width m_z on ``(seed + 2 * 0x9E3779B97F4A7C15) mod 2^64``
        (`syndrome_noise_seeds`), so that neither stream is the one `pauli_noise` or `bsc_noise` draws from `seed` itself.  The streams
        are indexed by global sample: rows `first_sample .. first_sample + B - 1` are what one process drawing all samples would get."""
        out = []
        with torch.cuda.device(self.device):
            for s, width in zip(self.syndrome_noise_seeds(seed), (self.m_x, self.m_z)):
                u = self._new((B, width), torch.uint8)
                check(_lib.lib().fgnn_bsc_noise(s, float(np.float32(q)), int(first_sample), B, width, _ptr(u), _stream(self.device)))
                out.append(u)
        return out[0], out[1]

    def bsc_noise(self, seed, p, first_sample, B):
        e = self._new((B, self.n), torch.uint8)
        with torch.cuda.device(self.device):
            check(_lib.lib().fgnn_bsc_noise(int(seed), float(np.float32(p)), int(first_sample), B, self.n, _ptr(e),
                                            _stream(self.device)))
        return e

    # ---- GNN_BP4 -----------------------------------------------------------------------------------------
    def gnn_bp4_decode(self, weights, synd_x, synd_z, num_iter, return_logits=True, workspace=None):
        B, synd_x, synd_z = self._syndromes_in(synd_x, synd_z)
        nbytes = _lib.lib().fgnn_gnnbp4_weights_workspace_bytes(self.handle, weights.handle, B)
        if workspace is None:
            workspace = self._new((nbytes,), torch.uint8)
        xh = self._new((B, self.n), torch.uint8)
        zh = self._new((B, self.n), torch.uint8)
        llr = self._new((B, 3, self.n), torch.float32)
        xl = self._new((num_iter, B, self.m_z + self.rows_lz), torch.float32) if return_logits else None
        zl = self._new((num_iter, B, self.m_x + self.rows_lx), torch.float32) if return_logits else None
        check(_lib.lib().fgnn_gnnbp4_decode(self.handle, weights.handle, int(num_iter), _ptr(synd_x), _ptr(synd_z), B, _ptr(xh),
                                            _ptr(zh), _ptr(llr), _ptr(xl), _ptr(zl), _ptr(workspace), workspace.numel(),
                                            _stream(self.device)))
        return dict(x_hat=xh, z_hat=zh, llr=llr, x_logit_all=xl, z_logit_all=zl)

    def _gnn_bp4_trainable(self, weights):
        """The reverse pass exists for runtime-shaped handles with sum / mean and no attributes; anything else is refused here,
        before any kernel is launched."""
        if weights.config[3] in ("max", "min"):
            raise NotImplementedError(f"reduce_op {weights.config[3]!r} is not differentiable here: the GNN_BP4 reverse pass implements sum and mean")
        if weights.config[6]:
            raise NotImplementedError("use_attributes=True is not differentiable here: the GNN_BP4 reverse pass has no attribute gradients")
        if not weights.general:
            raise ValueError("the GNN_BP4 tape and reverse pass take a runtime-shaped weight set: GnnBp4Weights(..., force_general=True)")

    def gnn_bp4_tape_bytes(self, weights, num_iter, B):
        self._gnn_bp4_trainable(weights)
        nbytes = C.c_size_t()
        check(_lib.lib().fgnn_gnnbp4_tape_bytes(self.handle, weights.handle, int(num_iter), int(B), C.byref(nbytes)))
        return int(nbytes.value)

    def gnn_bp4_backward_workspace_bytes(self, weights, B):
        self._gnn_bp4_trainable(weights)
        nbytes = C.c_size_t()
        check(_lib.lib().fgnn_gnnbp4_backward_workspace_bytes(self.handle, weights.handle, int(B), C.byref(nbytes)))
        return int(nbytes.value)

    def gnn_bp4_forward_tape(self, weights, synd_x, synd_z, num_iter, tape=None):
        """GNN_BP4.call with a tape for `gnn_bp4_backward` (fgnn_gnnbp4_forward_tape): the soft syndromes of `gnn_bp4_decode` on the
        same runtime-shaped weight set, bit for bit, and the activation tape (a float32 tensor; pass one to reuse it)."""
        self._gnn_bp4_trainable(weights)
        T = int(num_iter)
        B, synd_x, synd_z = self._syndromes_in(synd_x, synd_z)
        if tape is None:
            tape = self._new((self.gnn_bp4_tape_bytes(weights, T, B) // 4,), torch.float32)
        xl = self._new((T, B, self.m_z + self.rows_lz), torch.float32)
        zl = self._new((T, B, self.m_x + self.rows_lx), torch.float32)
        with torch.cuda.device(self.device):
            check(_lib.lib().fgnn_gnnbp4_forward_tape(self.handle, weights.handle, T, _ptr(synd_x), _ptr(synd_z), B, _ptr(xl), _ptr(zl),
                                                      _ptr(tape), tape.numel() * 4, _stream(self.device)))
        return dict(x_logit_all=xl, z_logit_all=zl, tape=tape)

    def gnn_bp4_backward(self, weights, synd_x, synd_z, num_iter, tape, grad_x_logit_all, grad_z_logit_all, workspace=None):
        """d loss / d (every Dense array of `weights`), summed over the batch, from d loss / d (x_logit_all, z_logit_all) of
        `gnn_bp4_forward_tape` (either may be None) — fgnn_gnnbp4_backward.  Returns one flat float32 tensor in weight-list order."""
        self._gnn_bp4_trainable(weights)
        T = int(num_iter)
        B, synd_x, synd_z = self._syndromes_in(synd_x, synd_z)
        grad_x_logit_all = self._opt(grad_x_logit_all, (T, B, self.m_z + self.rows_lz), torch.float32, "grad_x_logit_all")
        grad_z_logit_all = self._opt(grad_z_logit_all, (T, B, self.m_x + self.rows_lx), torch.float32, "grad_z_logit_all")
        count = C.c_int()
        check(_lib.lib().fgnn_gnnbp4_grad_count(self.handle, weights.handle, C.byref(count)))
        if workspace is None:
            workspace = self._new((self.gnn_bp4_backward_workspace_bytes(weights, B),), torch.uint8)
        grad = self._new((count.value,), torch.float32)
        with torch.cuda.device(self.device):
            check(_lib.lib().fgnn_gnnbp4_backward(self.handle, weights.handle, T, _ptr(synd_x), _ptr(synd_z), B, _ptr(tape),
                                                  tape.numel() * 4, _ptr(grad_x_logit_all), _ptr(grad_z_logit_all), _ptr(grad),
                                                  count.value, _ptr(workspace), workspace.numel(), _stream(self.device)))
        return grad


GNNBP4_SHAPES = ([(40, 40), (40,), (40, 20), (20,)] * 2 + [(41, 40), (40,), (40, 20), (20,)] * 2 + [(40, 40), (40,), (40, 20), (20,)] * 2
                 + [(60, 40), (40,), (40, 20), (20,)] + [(20, 3), (3,)])


SHIPPED_GNNBP4_CONFIG = (20, 40, 2, "mean", "tanh", True, False, 0, 0)


def gnnbp4_weight_shapes(graph_or_code, config):
    """Shapes of a GNN_BP4 weight list (order of fgnn.h: 7 MLPs x L Dense, _llr_inv_embed, then the 7 attribute arrays) for
    config = (num_embed_dims, num_hidden_units, num_mlp_layers, reduce_op, activation, use_bias, use_attributes,
    node_attribute_dims, msg_attribute_dims)."""
    D, H, L, _, _, bias, attr, An, Am = config
    if not attr:
        An = Am = 0
    nin = [2 * D + Am] * 2 + [2 * D + An + 1] * 2 + [2 * D + Am] * 2 + [3 * D + An]
    shapes = []
    for q in range(7):
        for k in range(L):
            K, J = (nin[q] if k == 0 else H), (D if k == L - 1 else H)
            shapes.append((K, J))
            if bias:
                shapes.append((J,))
    shapes.append((D, 3))
    if bias:
        shapes.append((3,))
    if attr:
        g = graph_or_code
        if hasattr(g, "hx"):
            hx, hz = np.asarray(g.hx), np.asarray(g.hz)
            n, mx, mz, ex, ez = hx.shape[1], hx.shape[0], hz.shape[0], int(hx.sum()), int(hz.sum())
        else:
            n, mx, mz, ex, ez = g.n, g.m_x, g.m_z, g.E_x, g.E_z
        shapes += [(mx, An), (mz, An), (ex, Am), (ez, Am), (n, An), (ex, Am), (ez, Am)]
    return shapes


class GnnBp4Weights:
    """Device copy of one GNN_BP4 parameter set (order of fgnn.h).  The benchmark configuration (20, 40, 2, mean, tanh, bias, no
    attributes: 30 arrays) runs the MFMA kernel; any other constructor setting — pass ``config`` and the ``graph`` (edge attributes
    are re-ordered for it) — a runtime-shaped kernel (fgnn_gnnbp4_weights_create_general)."""

    def __init__(self, arrays, device, config=SHIPPED_GNNBP4_CONFIG, graph=None, force_general=False):
        arrays = [np.ascontiguousarray(a, dtype=np.float32) for a in arrays]
        D, H, L, red, act, bias, attr, An, Am = config
        if red not in REDUCE_OPS:
            raise ValueError("unknown reduce operation")  # gnn.py:568
        if act not in ACTIVATIONS:
            raise NotImplementedError(f"activation {act!r}: the HIP kernels implement {sorted(k for k in ACTIVATIONS if k)}")
        self.config = (int(D), int(H), int(L), red, act, bool(bias), bool(attr), int(An) if attr else 0, int(Am) if attr else 0)
        self.general = force_general or self.config != SHIPPED_GNNBP4_CONFIG
        self.arrays = arrays
        self.device = _resolve_device(device)
        h = C.c_void_p()
        if not self.general:
            if [a.shape for a in arrays] != GNNBP4_SHAPES:
                raise ValueError(f"GNN_BP4 weights must have shapes {GNNBP4_SHAPES}")
            ptrs = (C.c_void_p * 30)(*[a.ctypes.data for a in arrays])
            check(_lib.lib().fgnn_gnnbp4_weights_create(ptrs, 20, 40, self.device.index, C.byref(h)))
        else:
            if graph is None:
                raise ValueError("a runtime-shaped GNN_BP4 weight set is built for a graph: pass graph=")
            shapes = gnnbp4_weight_shapes(graph, self.config)
            if [a.shape for a in arrays] != shapes:
                raise ValueError(f"GNN_BP4 weights must have shapes {shapes}, got {[a.shape for a in arrays]}")
            cfg = (C.c_int * 9)(self.config[0], self.config[1], self.config[2], REDUCE_OPS[red], ACTIVATIONS[act], int(bool(bias)),
                                int(bool(attr)), self.config[7], self.config[8])
            ptrs = (C.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])
            check(_lib.lib().fgnn_gnnbp4_weights_create_general(graph.handle, cfg, ptrs, len(arrays), C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().fgnn_gnnbp4_weights_destroy(self.handle)
        except Exception:
            pass
