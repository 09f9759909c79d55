"""The Python frame the code-based decoders and the sharded evaluation models share: input conversion of the ``QLDPCBPDecoder`` call,
graph attachment, the float32 priors, and the cursor of a sample stream sharded over ranks.  Private: nothing here is exported from
the package.  A decoder module writes its constructor checks, its ``decode`` (one `TannerGraph` call) and its docstrings; the rest
comes from `CodeDecoder`, and its evaluation model from `DepolarizingBP4Model`.
"""
import numpy as np
import torch

from ._lib import CN_TYPES


def depolarizing_llr(p0):
    """``log(3(1-p0)/p0)`` in float32 arithmetic: the LLR of each of X, Y, Z under depolarizing noise of rate ``p0``."""
    p0 = np.float32(p0)
    return float(np.log(np.float32(3.0) * (np.float32(1.0) - p0) / p0, dtype=np.float32))


def bsc_logit(p):
    """``-log((1-p)/p)`` in float32 arithmetic: the logit ``log p(1)/p(0)`` of a bit flipped with probability ``p``."""
    p = np.float32(p)
    return float(-np.log((np.float32(1.0) - p) / p, dtype=np.float32))


def syndrome_in(s, rows, device, batch_size=None):
    """A syndrome ``[rows, batch_size]`` of any number type as the library's ``[batch_size, rows]`` uint8 bits (``value & 1``)."""
    s = torch.as_tensor(s, device=device)
    if s.dim() != 2 or s.shape[0] != rows:
        raise ValueError(f"syndrome must have shape [{rows}, batch_size], got {tuple(s.shape)}")
    if batch_size is not None and s.shape[1] != batch_size:
        raise ValueError('batch sizes of llr_ch and the syndromes differ.')
    return (s.to(torch.int64) & 1).to(torch.uint8).t().contiguous()


def llr_ch_in(llr_ch, n, device):
    """The channel LLRs of a ``QLDPCBPDecoder``-style call: float32 ``[batch_size, 3, n]``, returned contiguous."""
    llr_ch = torch.as_tensor(llr_ch, device=device)
    if llr_ch.dtype != torch.float32:
        raise TypeError('Invalid input dtype.')
    if llr_ch.shape[-1] != n:
        raise ValueError('Last dimension must be of length n.')
    if llr_ch.dim() != 3 or llr_ch.shape[1] != 3:
        raise ValueError('llr_ch must have shape [batch_size, 3, n].')
    return llr_ch.contiguous()


def quaternary_in(llr_ch, syndrome_x, syndrome_z, n, rows_x, rows_z, device):
    """``(llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs])`` as ``(llr_ch, synd_x [bs,m_x], synd_z [bs,m_z])`` for the graph;
    checked in this order: llr_ch, then per syndrome (x before z) its shape and its batch size."""
    llr_ch = llr_ch_in(llr_ch, n, device)
    bs = llr_ch.shape[0]
    return llr_ch, syndrome_in(syndrome_x, rows_x, device, bs), syndrome_in(syndrome_z, rows_z, device, bs)


def alpha_list(alphas, max_alphas, num_iter, factor, cn_type):
    """The constructor checks of the decoders that sweep a list of message strengths; returns the list as a tuple of floats."""
    alphas = tuple(float(x) for x in alphas)
    if not 1 <= len(alphas) <= max_alphas:
        raise ValueError(f"alphas must hold 1 .. {max_alphas} values")
    if not all(np.isfinite(x) and x > 0 for x in alphas):
        raise ValueError("every alpha must be finite and positive")
    if not isinstance(num_iter, (int, np.integer)) or num_iter < 1:
        raise ValueError("num_iter must be a positive integer")
    if not (np.isfinite(float(factor)) and float(factor) > 0):
        raise ValueError("factor must be finite and positive")
    if cn_type not in CN_TYPES:
        raise ValueError("Unknown node type.")
    return alphas


def schedule_in(schedule, layers, serial):
    """The constructor checks of a decoder that runs 'flooding' or the serial schedule named ``serial`` ('layered', 'serial'); made
    before the decoder builds a graph, so a refusal touches no device."""
    if not isinstance(schedule, str) or schedule not in ("flooding", serial):
        raise ValueError(f"schedule must be 'flooding' or {serial!r}, got {schedule!r}")
    if layers is not None and schedule != serial:
        raise ValueError(f"layers= belongs to schedule={serial!r}")


def install_layering(graph, schedule, layers, serial, getter, setter):
    """A decoder in the serial schedule hands ``layers`` to the graph's ``setter`` (`set_layers`, `set_bit_layers`, `set_qubit_layers`;
    None: the greedy layering) — unless it names none and the graph, shared with another decoder, has one already (``getter``)."""
    if schedule == serial and (layers is not None or getattr(graph, getter)()[0] == 0):
        getattr(graph, setter)(layers)


def alias(name):
    """A read/write property that is another attribute under a second (historical) name."""
    return property(lambda self: getattr(self, name), lambda self, value: setattr(self, name, value))


class CodeDecoder:
    """Base of the decoders built on a CSS code's `TannerGraph` and called like ``QLDPCBPDecoder``.  The subclass validates its
    arguments, calls `_attach` and provides ``decode(synd_x, synd_z, ..., llr_ch=)`` whose result starts with ``x_hat, z_hat``."""

    def _attach(self, code, graph, device):
        """Take ``graph`` (or build the code's own, with code.hx_perp / code.hz_perp as row sets) and cache its sizes."""
        self._code = code
        if graph is None:
            from .graph import TannerGraph
            graph = TannerGraph(code, stage_one=False, device=device)
        self.graph = graph
        self._num_vns, self._num_cns_x, self._num_cns_z = graph.n, graph.m_x, graph.m_z
        self.last_stats = None

    code = property(lambda self: self._code)
    num_vns = property(lambda self: self._num_vns)

    def __call__(self, inputs):
        llr_ch, syndrome_x, syndrome_z = inputs
        llr_ch, synd_x, synd_z = quaternary_in(llr_ch, syndrome_x, syndrome_z, self._num_vns, self._num_cns_x, self._num_cns_z,
                                               self.graph.device)
        x_hat, z_hat = self.decode(synd_x, synd_z, llr_ch=llr_ch)[:2]
        return x_hat.to(torch.int64), z_hat.to(torch.float64)

    call = __call__


class ShardedModel:
    """The cursor of a counter-based sample stream that ``world_size`` ranks draw from in turn: a batch of B takes the global samples
    ``_next + rank * B ..`` and moves ``_next`` (a plain int; assign it to rewind) on by ``world_size * B``."""

    def _shard(self, seed, rank, world_size):
        self.seed, self.rank, self.world_size, self._next = int(seed), int(rank), int(world_size), 0

    def next_sample_range(self, batch_size):
        """``(first, last)``: the half-open range of global sample indices this rank's next batch will draw."""
        first = self._next + self.rank * int(batch_size)
        return first, first + int(batch_size)

    def _take(self, B):
        """First global sample index of this rank's batch of ``B``; the stream moves on past all ranks' batches."""
        first = self._next + self.rank * B
        self._next += self.world_size * B
        return first


class DepolarizingBP4Model(ShardedModel):
    """``model(batch_size, p)`` → ``(s_hat, ls_hat)`` of a `CodeDecoder` under depolarizing noise: noise, its two syndromes, the decoder
    with the prior ``log(3(1-p0)/p0)``, the residual.  A subclass may change the syndromes (`_measure`) and how ``decode`` is called
    (`_decode`)."""

    def __init__(self, code, decoder, p0=None, *, seed=0x5EED, rank=0, world_size=1):
        self.code, self.decoder, self.p0 = code, decoder, p0
        self.graph = decoder.graph
        self._shard(seed, rank, world_size)
        self.last_noise_x = self.last_noise_z = self.last_x_hat = self.last_z_hat = self.last_stats = None
        self.last_num_unsolved = 0

    def _measure(self, sx, sz, first, B):
        """The syndromes the decoder sees, from the exact ones of samples ``first .. first + B - 1``."""
        return sx, sz

    def _decode(self, sx, sz, llr_const, first):
        """``(x_hat, z_hat, stats)`` of one batch."""
        return self.decoder.decode(sx, sz, llr_const=llr_const)

    def __call__(self, batch_size, ebno_db=None, **kw):
        p = float(kw.get("p", ebno_db))
        B, g = int(batch_size), self.graph
        first = self._take(B)
        llr_const = depolarizing_llr(p if self.p0 is None else self.p0)
        ex, ez = g.pauli_noise(self.seed, p, first, B)
        sx, sz = self._measure(*g.syndrome(ex, ez), first, B)
        x_hat, z_hat, stats = self._decode(sx, sz, llr_const, first)
        self.last_noise_x, self.last_noise_z, self.last_x_hat, self.last_z_hat, self.last_stats = ex, ez, x_hat, z_hat, stats
        self.last_num_unsolved = int((stats[:, 0] == 0).sum().item())
        s_hat, ls_hat, _ = g.residual(ex, ez, x_hat, z_hat, want_arrays=True)
        return s_hat, ls_hat

    call = __call__
