"""Relay-BP on MI355X: binary min-sum BP with per-bit memory strengths, run as a chain of legs in one kernel launch.

Mueller et al., "Improved belief propagation is sufficient for real-time decoding of quantum memories" (2025).  The algorithm is
stated at `fgnn_relay_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_relay.hip.  It needs no training and no
matrix inversion and runs on any binary check matrix that fits the LDS-resident layout.

Relay-BP4 (`RelayBP4Decoder`, `BP4_Relay_Model`) is the same scheme on the quaternary decoder: the memory term on each of a qubit's
three LLRs, both Tanner graphs of a CSS code in one kernel (`fgnn_relay4_decode`, feedback_gnn_amd/csrc/fgnn_relay4.hip).
"""
import numpy as np
import torch

from ._frontend import CodeDecoder, DepolarizingBP4Model, ShardedModel, alias, bsc_logit, install_layering, schedule_in
from .decoding import _adopt_bit_layers, _binary_graph


def _relay_schedule(pre_iter, num_sets, set_max_iter, gamma_dist_interval, stop_nconv):
    """The validation both decoder classes share; returns the interval as floats."""
    for name, val in (("pre_iter", pre_iter), ("set_max_iter", set_max_iter), ("stop_nconv", stop_nconv)):
        if not isinstance(val, (int, np.integer)) or val < 1:
            raise ValueError(f"{name} must be a positive integer")
    if not isinstance(num_sets, (int, np.integer)) or num_sets < 0:
        raise ValueError("num_sets cannot be negative")
    lo, hi = (float(x) for x in gamma_dist_interval)
    if not lo <= hi:
        raise ValueError("gamma_dist_interval must be (low, high) with low <= high")
    return lo, hi


def _draw_gamma(gamma0, num_sets, n, lo, hi, seed):
    """[1 + num_sets, n] float32: gamma0 on the first leg, then uniform draws of np.random.default_rng(seed)."""
    gamma = np.empty((1 + num_sets, n), np.float32)
    gamma[0] = np.float32(gamma0)
    gamma[1:] = np.random.default_rng(seed).uniform(lo, hi, size=(num_sets, n)).astype(np.float32)
    return gamma


class RelayBPDecoder:
    """``RelayBPDecoder(pcm, gamma0=0.125, pre_iter=80, num_sets=60, set_max_iter=60, gamma_dist_interval=(-0.24, 0.66),
    stop_nconv=1, normalization_factor=1.0, seed=0)``.  The first leg runs up to ``pre_iter`` iterations with memory strength
    ``gamma0`` on every bit; each of the ``num_sets`` further legs runs up to ``set_max_iter`` iterations with strengths drawn once,
    at construction, uniformly in ``gamma_dist_interval`` from ``np.random.default_rng(seed)``.  Decoding stops after ``stop_nconv``
    solutions and keeps the one of lowest weight.

    Call ``decoder((llr_ch[bs,n], syndrome[m,bs]))`` as ``LDPCBPDecoder(is_syndrome=True, hard_out=True)``: ``llr_ch`` are logits
    (log p(1)/p(0)), the result is the estimate ``e_hat[bs,n]`` (0/1 floats).  ``last_stats[bs,4]`` (int32) = solutions found, weight
    of the estimate (sum of rint(1024 * |clipped logit|) signed as the prior), its leg and its iteration within the leg.

    ``schedule="flooding"`` (the default) runs every leg as flooding min-sum (`fgnn_relay_decode`); ``schedule="layered"`` runs the legs
    in the layered (serial) check schedule (`fgnn_relay_decode_layered`), on the bit layering of the graph: ``layers`` [m] gives every
    check its layer and is handed to ``graph.set_bit_layers`` (None: the layering the graph has, or the greedy one)."""

    def __init__(self, pcm, gamma0=0.125, pre_iter=80, num_sets=60, set_max_iter=60, gamma_dist_interval=(-0.24, 0.66), stop_nconv=1,
                 normalization_factor=1.0, seed=0, device=None, graph=None, schedule="flooding", layers=None):
        pcm = np.asarray(pcm.toarray() if hasattr(pcm, "toarray") else pcm)
        if not np.array_equal(pcm, pcm.astype(bool)):
            raise AssertionError('PC matrix must be binary.')
        schedule_in(schedule, layers, "layered")
        lo, hi = _relay_schedule(pre_iter, num_sets, set_max_iter, gamma_dist_interval, stop_nconv)
        self.schedule = schedule
        self._pcm = pcm
        self.pre_iter, self.num_sets, self.set_max_iter, self.stop_nconv = int(pre_iter), int(num_sets), int(set_max_iter), int(stop_nconv)
        self.gamma0, self.gamma_dist_interval, self.seed = float(gamma0), (lo, hi), int(seed)
        self.normalization_factor = float(normalization_factor)
        self.graph = graph if graph is not None else _binary_graph(pcm, None, device)
        self._num_vns, self._num_cns = self.graph.n, self.graph.m_x
        self.gamma = _draw_gamma(self.gamma0, self.num_sets, self._num_vns, lo, hi, self.seed)
        install_layering(self.graph, schedule, layers, "layered", "bit_layers", "set_bit_layers")
        self.last_stats = None

    pcm = property(lambda self: self._pcm)
    num_cns = property(lambda self: self._num_cns)
    num_vns = property(lambda self: self._num_vns)
    num_legs = property(lambda self: 1 + self.num_sets)

    @property
    def gamma(self):
        """The memory strengths [1 + num_sets, n] (float32, on the device)."""
        return self._gamma

    @gamma.setter
    def gamma(self, value):
        value = torch.as_tensor(np.asarray(value.cpu() if isinstance(value, torch.Tensor) else value, dtype=np.float32))
        if tuple(value.shape) != (1 + self.num_sets, self._num_vns):
            raise ValueError(f"gamma must have shape {(1 + self.num_sets, self._num_vns)}, got {tuple(value.shape)}")
        self._gamma = value.to(self.graph.device).contiguous()

    def decode(self, synd, llr_ch=None, llr_const=0.0, B=None):
        """Estimates and stats for syndromes [B, m] (uint8, device) under per-bit logits ``llr_ch`` [B, n] or one logit for every bit."""
        hard, stats = self._entry(self.graph)(synd, self._gamma, self.pre_iter, self.set_max_iter, self.stop_nconv,
                                              self.normalization_factor, llr_ch=llr_ch, llr_const=llr_const, B=B)
        self.last_stats = stats
        return hard, stats

    def _entry(self, graph):
        """The wrapper of `graph` that runs this decoder's schedule."""
        return graph.relay_decode_layered if self.schedule == "layered" else graph.relay_decode

    def __call__(self, inputs):
        g = self.graph
        llr_ch, syndrome = inputs
        syndrome = torch.as_tensor(syndrome, device=g.device)
        if syndrome.dim() != 2 or syndrome.shape[0] != self._num_cns:
            raise ValueError(f"syndrome must have shape [{self._num_cns}, batch_size]")
        synd = (syndrome.to(torch.int64) & 1).to(torch.uint8).t().contiguous()
        llr_ch = torch.as_tensor(llr_ch, device=g.device)
        if llr_ch.dtype != torch.float32:
            raise TypeError('Invalid input dtype.')
        if llr_ch.shape[-1] != self._num_vns:
            raise ValueError('Last dimension must be of length n.')
        shape = llr_ch.shape
        hard, _ = self.decode(synd, llr_ch=llr_ch.reshape(-1, self._num_vns).contiguous())
        return hard.to(torch.float32).reshape(shape)

    call = __call__


class BP2_Relay_Model(ShardedModel):
    """``BP2_Relay_Model(pcm, logical_pcm, relay_decoder)``; ``model(batch_size, p)`` → ``(s_hat[bs,m], ls_hat[bs,rows(logical_pcm)])``,
    shaped like ``BP2_OSD_Model``: BSC(p) noise, its syndrome, Relay-BP.  ``s_hat = pcm·(noise xor estimate)`` is non-zero exactly on
    the samples for which no solution was found, ``ls_hat = logical_pcm·(noise xor estimate)``.  After a call ``last_noise``,
    ``last_estimate`` (uint8 [bs,n]), ``last_stats`` (int32 [bs,4]) and ``last_num_unsolved`` describe that batch.  The model follows
    its decoder's ``schedule``: under a layered decoder its graph takes the decoder's layering and the legs run layered."""

    def __init__(self, pcm, logical_pcm, relay_decoder, *, seed=0x5EED, rank=0, world_size=1):
        self.pcm, self.logical_pcm, self.relay_decoder = pcm, logical_pcm, relay_decoder
        self.graph = _binary_graph(pcm, logical_pcm, relay_decoder.graph.device)
        _adopt_bit_layers(self.graph, relay_decoder)  # a layered decoder: its layering on the model's own graph
        self._shard(seed, rank, world_size)
        self.last_noise = self.last_estimate = self.last_stats = None
        self.last_num_unsolved = 0

    def __call__(self, batch_size, ebno_db=None, **kw):
        p = float(kw.get("p", ebno_db))
        B, g, d = int(batch_size), self.graph, self.relay_decoder
        noise = g.bsc_noise(self.seed, p, self._take(B), B)
        zeros = torch.zeros_like(noise)
        synd, _ = g.syndrome(zeros, noise)
        noise_hat, stats = d._entry(g)(synd, d.gamma, d.pre_iter, d.set_max_iter, d.stop_nconv, d.normalization_factor,
                                       llr_const=bsc_logit(p), B=B)
        d.last_stats = stats
        self.last_noise, self.last_estimate, self.last_stats = noise, noise_hat, stats
        self.last_num_unsolved = int((stats[:, 0] == 0).sum().item())
        s_hat, ls_hat, _ = g.residual(noise, zeros, noise_hat, zeros, want_arrays=True)
        return s_hat[:, :g.m_z].contiguous(), ls_hat[:, :g.rows_hxp].contiguous()

    call = __call__


class RelayBP4Decoder(CodeDecoder):
    """``RelayBP4Decoder(code, gamma0=0.125, pre_iter=80, num_sets=60, set_max_iter=60, gamma_dist_interval=(-0.24, 0.66),
    stop_nconv=1, normalization_factor=1.0, seed=0)``: Relay-BP on the quaternary decoder.  The schedule and the memory strengths are
    `RelayBPDecoder`'s (one strength per qubit and leg, applied to the qubit's three LLRs); every leg is min-sum BP4 on both Tanner
    graphs of ``code``.  Decoding stops after ``stop_nconv`` solutions (estimates that reproduce both syndromes) and keeps the one of
    lowest weight.

    Call ``decoder((llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs]))`` as ``QLDPCBPDecoder``: the result is
    ``(x_hat, z_hat)`` [bs,n] in its dtypes (int64 and float64).  ``last_stats[bs,4]`` (int32) = solutions found, weight of the estimate
    (sum over the qubits of rint(1024 * clipped channel LLR) of the decided Pauli), its leg and its iteration within the leg."""

    def __init__(self, code, gamma0=0.125, pre_iter=80, num_sets=60, set_max_iter=60, gamma_dist_interval=(-0.24, 0.66), stop_nconv=1,
                 normalization_factor=1.0, seed=0, device=None, graph=None):
        lo, hi = _relay_schedule(pre_iter, num_sets, set_max_iter, gamma_dist_interval, stop_nconv)
        self.pre_iter, self.num_sets, self.set_max_iter, self.stop_nconv = int(pre_iter), int(num_sets), int(set_max_iter), int(stop_nconv)
        self.gamma0, self.gamma_dist_interval, self.seed = float(gamma0), (lo, hi), int(seed)
        self.normalization_factor = float(normalization_factor)
        self._attach(code, graph, device)
        self.gamma = _draw_gamma(self.gamma0, self.num_sets, self._num_vns, lo, hi, self.seed)

    num_legs = property(lambda self: 1 + self.num_sets)
    gamma = RelayBPDecoder.gamma

    def decode(self, synd_x, synd_z, llr_ch=None, llr_const=0.0):
        """Estimates and stats for syndromes [B, m_x] / [B, m_z] (uint8, device) under ``llr_ch`` [B, 3, n] or one LLR for everything."""
        x_hat, z_hat, stats = self.graph.relay4_decode(synd_x, synd_z, self._gamma, self.pre_iter, self.set_max_iter, self.stop_nconv,
                                                       self.normalization_factor, llr_ch=llr_ch, llr_const=llr_const)
        self.last_stats = stats
        return x_hat, z_hat, stats


class BP4_Relay_Model(DepolarizingBP4Model):
    """``BP4_Relay_Model(code, relay_decoder, p0=None)``; ``model(batch_size, p)`` → ``(s_hat[bs, m_z+m_x], ls_hat[bs,
    rows(hx_perp)+rows(hz_perp)])``, shaped like ``Sandwich_BP_GNN_Evaluation_Model``: depolarizing noise of rate ``p``, its two
    syndromes, Relay-BP4 with the prior ``log(3(1-p0)/p0)`` (``p0=None``: of ``p`` itself).  ``s_hat`` is non-zero exactly on the samples
    for which no solution was found.  After a call ``last_noise_x``, ``last_noise_z``, ``last_x_hat``, ``last_z_hat`` (uint8 [bs,n]),
    ``last_stats`` (int32 [bs,4]) and ``last_num_unsolved`` describe that batch.  ``rank`` / ``world_size`` shard the sample stream."""

    def __init__(self, code, relay_decoder, p0=None, *, seed=0x5EED, rank=0, world_size=1):
        super().__init__(code, relay_decoder, p0, seed=seed, rank=rank, world_size=world_size)

    relay_decoder = alias("decoder")
