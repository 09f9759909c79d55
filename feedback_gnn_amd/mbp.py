"""BP4 with message-strength control on MI355X: MBP4 and its adaptive form AMBP4 (Kuo, Lai, "Exploiting degeneracy in belief
propagation decoding of quantum codes", npj Quantum Information, 2022), in the flooding schedule or in the paper's serial one.

A qubit's belief is formed from its incoming check messages scaled by ``1 / alpha``, while the message it sends back to a check has
that check's own contribution removed at full strength (the inhibition term); ``alpha < 1`` breaks the symmetric stalls that
degenerate codes cause.  AMBP4 tries a descending list of alphas and keeps the first whose estimate reproduces both syndromes.  The
algorithm is stated at `fgnn_mbp4_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_mbp4.hip: one launch, all
alphas of a codeword with its messages and decisions in LDS throughout.  It needs no training, no random numbers and no matrix
inversion.  The serial schedule visits the qubits one layer after the other, each seeing the messages the qubits before it have just
sent (`fgnn_mbp4_decode_serial`, feedback_gnn_amd/csrc/fgnn_mbp4_serial.hip); a layer holds qubits that share no check.
"""
import numpy as np
import torch

from ._frontend import CodeDecoder, DepolarizingBP4Model, alpha_list, install_layering, schedule_in

ALPHA_DEFAULTS = (1.0, 0.9, 0.8, 0.7, 0.6, 0.5)
MAX_ALPHAS = 64


def mbp4_tables(alphas, base):
    """``(factor, own)`` float32 arrays of `fgnn_mbp4_decode` for Kuo-Lai's MBP4: ``own[a] = float32(alpha_a)`` and ``factor[a] =
    float32(base) / float32(alpha_a)``, one IEEE float32 division."""
    own = np.asarray(alphas, dtype=np.float32).reshape(-1)
    factor = (np.float32(base) / own).astype(np.float32)
    return factor, own


class AMBP4Decoder(CodeDecoder):
    """``AMBP4Decoder(code, alphas=None, num_iter=64, cn_type="minsum", factor=0.8, restart=True, schedule="flooding",
    layers=None)``.  For every alpha of ``alphas``
    in turn (``None``: ``ALPHA_DEFAULTS``), BP4 with message strength alpha runs up to ``num_iter`` iterations with its check outputs
    multiplied by ``factor / alpha``, from zero messages or, with ``restart=False``, from the messages the alpha before left; the first
    estimate that reproduces both syndromes is the result.  One alpha is MBP4; ``alphas=(1.0,)`` is flooding BP4 that stops at its
    first solution.  ``schedule="serial"`` runs every alpha in Kuo and Lai's serial schedule (`TannerGraph.mbp4_decode_serial`);
    ``layers`` gives every qubit its layer and is handed to ``graph.set_qubit_layers`` (None: the layering the graph has, or the greedy
    one).

    Call ``decoder((llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs]))`` as ``QLDPCBPDecoder``: the result is
    ``(x_hat, z_hat)`` [bs,n] in its dtypes (int64 and float64).  ``last_stats[bs,4]`` (int32) = solution found, the index of the alpha
    of the last test, iterations run, and the iteration within that alpha of the last test; ``last_alpha[bs]`` (float32) = the alpha
    that solved the sample, NaN where none did."""

    def __init__(self, code, alphas=None, num_iter=64, cn_type="minsum", factor=0.8, restart=True, device=None, graph=None,
                 schedule="flooding", layers=None):
        schedule_in(schedule, layers, "serial")
        alphas = alpha_list(ALPHA_DEFAULTS if alphas is None else alphas, MAX_ALPHAS, num_iter, factor, cn_type)
        self.alphas, self.num_iter, self.cn_type, self.factor, self.restart = alphas, int(num_iter), cn_type, float(factor), bool(restart)
        self.factors, self.owns = mbp4_tables(alphas, factor)
        if not np.isfinite(self.factors).all():
            raise ValueError("factor / alpha must be finite in float32")
        self._attach(code, graph, device)
        self.schedule = schedule
        install_layering(self.graph, schedule, layers, "serial", "qubit_layers", "set_qubit_layers")
        self.last_alpha = None

    def solving_alpha(self, stats):
        """[B] float32: the alpha of the attempt in which the sample was solved (``stats[:, 1]``), NaN for an unsolved sample."""
        table = torch.from_numpy(self.owns).to(stats.device)
        alpha = table[stats[:, 1].long()]
        return torch.where(stats[:, 0] > 0, alpha, torch.full_like(alpha, float("nan")))

    def decode(self, synd_x, synd_z, llr_ch=None, llr_const=0.0, first_sample=0, seed=None):
        """Estimates and stats for syndromes [B, m_x] / [B, m_z] (uint8, device) under ``llr_ch`` [B, 3, n] or one LLR for everything.
        ``first_sample`` and ``seed`` are taken and ignored, so that the decoder can stand where a ``BP4FeedbackDecoder`` does: AMBP4
        draws nothing."""
        run = self.graph.mbp4_decode if self.schedule == "flooding" else self.graph.mbp4_decode_serial
        x_hat, z_hat, stats = run(synd_x, synd_z, self.factors, self.owns, self.num_iter, self.num_iter, self.cn_type, restart=self.restart,
                                llr_ch=llr_ch, llr_const=llr_const)
        self.last_stats, self.last_alpha = stats, self.solving_alpha(stats)
        return x_hat, z_hat, stats


class BP4_AMBP_Model(DepolarizingBP4Model):
    """``BP4_AMBP_Model(code, decoder, p0=None)``; ``model(batch_size, p)`` → ``(s_hat[bs, m_z+m_x], ls_hat[bs,
    rows(hx_perp)+rows(hz_perp)])``, shaped like ``BP4_Feedback_Model``: depolarizing noise of rate ``p`` from the stream of ``seed``,
    its two syndromes, AMBP4 in the decoder's schedule under the prior ``log(3(1-p0)/p0)`` (``p0=None``: of ``p`` itself).  ``s_hat`` is non-zero exactly on the
    samples for which no solution was found.  After a call ``last_noise_x``, ``last_noise_z``, ``last_x_hat``, ``last_z_hat`` (uint8
    [bs,n]), ``last_stats`` (int32 [bs,4]), ``last_alpha`` (float32 [bs]) and ``last_num_unsolved`` describe that batch.  ``rank`` /
    ``world_size`` shard the sample stream by global sample index: a shard decodes its samples exactly as a single process would."""

    last_alpha = None

    def _decode(self, sx, sz, llr_const, first):
        out = self.decoder.decode(sx, sz, llr_const=llr_const)
        self.last_alpha = self.decoder.last_alpha
        return out
