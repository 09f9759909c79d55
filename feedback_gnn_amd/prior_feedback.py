"""BP4 with hand-written prior feedback on MI355X: the two rules the learned feedback of the GNN (arXiv 2310.17758) is measured against.

When BP4 has run its iterations without a solution, the unsatisfied checks of its last estimate choose qubits whose channel LLRs are
changed, and BP4 runs again:
  "perturb"   random perturbation (Poulin, Chung, "On the iterative decoding of sparse quantum codes", 2008): every qubit on an
              unsatisfied check gets its three LLRs lowered by seeded random amounts up to ``strength``;
  "enhanced"  enhanced feedback (Wang, Sanders, Poulin, "Enhanced feedback iterative decoding of sparse quantum codes", 2012): at one
              qubit of one unsatisfied check the two Paulis that anticommute with the check are made likelier or less likely by
              ``strength``, as the measured syndrome bit demands.
The algorithm is stated at `fgnn_bp4fb_decode` in include/fgnn.h; the kernel is feedback_gnn_amd/csrc/fgnn_bp4fb.hip: one launch, all
attempts of a codeword with its messages, decisions and marks in LDS throughout.  Neither rule needs training or a matrix inversion.
"""
import numpy as np

from ._frontend import CodeDecoder, DepolarizingBP4Model
from ._lib import CN_TYPES, FB_RULES

# attempt_iter, max_attempts, strength where the constructor gets None: from a CPU prototype on [[882,24]] at p = 0.10
RULE_DEFAULTS = {"perturb": (8, 40, 2.0), "enhanced": (16, 20, 10.0)}


class BP4FeedbackDecoder(CodeDecoder):
    """``BP4FeedbackDecoder(code, rule="perturb", pre_iter=32, attempt_iter=None, max_attempts=None, strength=None, restart=False,
    cn_type="minsum", normalization_factor=0.8, seed=0x5EED)``.  BP4 runs up to ``pre_iter`` iterations; while no estimate reproduces
    both syndromes, up to ``max_attempts`` times, ``rule`` re-initialises the priors from the channel LLRs and the unsatisfied checks
    and BP4 runs up to ``attempt_iter`` iterations more, from the messages it has or, with ``restart=True`` (what the enhanced-feedback
    paper does), from zero messages.  ``None`` takes the rule's default: perturb (8, 40, 2.0), enhanced (16, 20, 10.0).

    Call ``decoder((llr_ch[bs,3,n], syndrome_x[m_x,bs], syndrome_z[m_z,bs]))`` as ``QLDPCBPDecoder``: the result is
    ``(x_hat, z_hat)`` [bs,n] in its dtypes (int64 and float64).  ``last_stats[bs,4]`` (int32) = solution found, feedback steps made,
    iterations run, and the iteration within its attempt of the last test.  The rules draw from the Philox stream of ``seed`` at the
    sample indices ``first_sample`` .. of ``decode``, apart from the channel noise of the same seed."""

    def __init__(self, code, rule="perturb", pre_iter=32, attempt_iter=None, max_attempts=None, strength=None, restart=False,
                 cn_type="minsum", normalization_factor=0.8, seed=0x5EED, device=None, graph=None):
        if rule not in FB_RULES:
            raise ValueError('rule must be "perturb" or "enhanced"')
        d_iter, d_attempts, d_strength = RULE_DEFAULTS[rule]
        attempt_iter = d_iter if attempt_iter is None else attempt_iter
        max_attempts = d_attempts if max_attempts is None else max_attempts
        strength = d_strength if strength is None else strength
        for name, val in (("pre_iter", pre_iter), ("attempt_iter", attempt_iter)):
            if not isinstance(val, (int, np.integer)) or val < 1:
                raise ValueError(f"{name} must be a positive integer")
        if not isinstance(max_attempts, (int, np.integer)) or not 0 <= max_attempts <= 65535:
            raise ValueError("max_attempts must be an integer in 0 .. 65535")
        if not (np.isfinite(float(strength)) and float(strength) >= 0):
            raise ValueError("strength must be finite and cannot be negative")
        if cn_type not in CN_TYPES:
            raise ValueError("Unknown node type.")
        self.rule, self.pre_iter, self.attempt_iter, self.max_attempts = rule, int(pre_iter), int(attempt_iter), int(max_attempts)
        self.strength, self.restart, self.seed = float(strength), bool(restart), int(seed)
        self.cn_type, self.normalization_factor = cn_type, float(normalization_factor)
        self._attach(code, graph, device)

    def decode(self, synd_x, synd_z, llr_ch=None, llr_const=0.0, first_sample=0, seed=None):
        """Estimates and stats for syndromes [B, m_x] / [B, m_z] (uint8, device) under ``llr_ch`` [B, 3, n] or one LLR for everything;
        row b is decoded as global sample ``first_sample + b`` of the stream of ``seed`` (None: the decoder's)."""
        x_hat, z_hat, stats = self.graph.bp4fb_decode(synd_x, synd_z, self.rule, self.pre_iter, self.attempt_iter, self.max_attempts,
                                                      self.strength, self.cn_type, self.normalization_factor, restart=self.restart,
                                                      seed=self.seed if seed is None else seed, first_sample=first_sample,
                                                      llr_ch=llr_ch, llr_const=llr_const)
        self.last_stats = stats
        return x_hat, z_hat, stats


class BP4_Feedback_Model(DepolarizingBP4Model):
    """``BP4_Feedback_Model(code, decoder, p0=None)``; ``model(batch_size, p)`` → ``(s_hat[bs, m_z+m_x], ls_hat[bs,
    rows(hx_perp)+rows(hz_perp)])``, shaped like ``BP4_GD_Model``: depolarizing noise of rate ``p``, its two syndromes, BP4 with prior
    feedback under the prior ``log(3(1-p0)/p0)`` (``p0=None``: of ``p`` itself).  The feedback draws use the model's ``seed`` and the
    batch's global sample indices, so a shard decodes its samples exactly as a single process would.  ``s_hat`` is non-zero exactly on
    the samples for which no solution was found.  After a call ``last_noise_x``, ``last_noise_z``, ``last_x_hat``, ``last_z_hat`` (uint8
    [bs,n]), ``last_stats`` (int32 [bs,4]) and ``last_num_unsolved`` describe that batch.  ``rank`` / ``world_size`` shard the sample
    stream."""

    def _decode(self, sx, sz, llr_const, first):
        return self.decoder.decode(sx, sz, llr_const=llr_const, first_sample=first, seed=self.seed)
