"""Iteration 0 of a BP4 decode that starts from zero messages (msg_init = None: every decoder of every sandwich).

The degree-regular kernels do not run that iteration edge by edge.  With one constant channel LLR and the phi rule it is evaluated in
closed form, once per thread; with per-qubit channel LLRs its qubit phase is peeled: no message is read and one log-sum-exp per qubit
and side gives the side's messages.  Both are chosen by the LAUNCH ARGUMENTS (msg_init, llr_ch, num_iter, the check rule), never by
the data, in the fixed dataflow as with the exact shortcuts on, and both execute the oracle's float operations: every output must
equal the C oracle's bit for bit — marginals, decisions, soft syndromes and final messages — at num_iter = 0 (neither form may
run), 1 (the decode ends right after it), 2 and 3 (its messages feed the generic loop).  Runtime-degree graphs, the other check rules
with a constant LLR, restarts (msg_init given) and the one-launch trace keep the generic path and are held to the same oracle here.
"""
import numpy as np
import pytest

from helpers import WEIGHTS_882, gpu_graph, llr_const, oracle_library_forms, to_gpu

pytestmark = pytest.mark.gpu
SEED = 0x5EED
KEYS = ("llr", "x_logit", "z_logit", "msg_x", "msg_z", "x_hat", "z_hat")
# (saturation shortcut, fixed-point exit): the fixed dataflow, the exact shortcuts, and the detector on top (acts from num_iter = 3)
MODES = ((False, False), (True, False), (True, True))
# (code, batch): ibm72 — (3,3,6)-regular, several codewords per workgroup, a thread owns at most one node, padded last workgroup;
# [[882,24]] — one codeword per workgroup, a last partial trip per thread, at 3 and at 257 codewords; gb48 — the (4,4,8) kernels;
# Steane and the rotated surface code — irregular: the runtime-degree path
CASES = [("ibm72", 77), ("ghp882", 3), ("ghp882", 257), ("gb48", 21), ("steane", 9), ("rsurf3", 9)]


class _forms:
    """The qubit update's log-sum-exp form on the oracle and the GPU graph together; restored on exit."""

    def __init__(self, name, shared):
        self.og, self.gg, self.on = oracle_library_forms(name), gpu_graph(name), shared

    def __enter__(self):
        self.prev = self.gg.bp4_shared_lse
        self.og.set_vn_shared_lse(self.on)
        self.gg.set_bp4_shared_lse(self.on)
        return self.og, self.gg

    def __exit__(self, *exc):
        self.og.set_vn_shared_lse(self.prev)
        self.gg.set_bp4_shared_lse(self.prev)
        self.gg.set_saturation_shortcut(True)
        self.gg.set_fixed_point_exit(True)
        self.gg.set_launch(0, 0)


def _eq(o, g, what):
    for k in KEYS:
        a = o[k] if isinstance(o[k], np.ndarray) else o[k].cpu().numpy()
        b = g[k].cpu().numpy()
        assert a.tobytes() == b.tobytes(), f"{what} {k}: {int((a != b).sum())} of {a.size} differ, first at {np.argwhere(a != b)[:3].tolist()}"


def _syndromes(og, B, first):
    """Syndromes of depolarizing noise, then one row with every bit set and one with none (the closed form's signs are syndrome-driven)."""
    ex, ez = og.pauli_noise(SEED, 0.08, first, B)
    sx, sz = og.syndrome(ex, ez)
    sx, sz = sx.copy(), sz.copy()
    sx[-1], sz[-1] = 1, 1
    if B > 1:
        sx[-2], sz[-2] = 0, 0
    return sx, sz


def _channel_llrs(B, n, seed):
    """Per-qubit LLRs with zeros of both signs, negatives and magnitudes beyond the softplus / phi / log-sum-exp thresholds."""
    rng = np.random.RandomState(seed)
    llr = rng.uniform(-4.0, 6.0, size=(B, 3, n)).astype(np.float32)
    specials = np.array([0.0, -0.0, -3.5, 13.95, -13.95, 16.635532, 16.7, -17.0, 20.0, 20.5, -25.0, 37.5, 88.0, -90.0], np.float32)
    pick = rng.rand(B, 3, n) < 0.15
    llr[pick] = specials[rng.randint(0, len(specials), size=int(pick.sum()))]
    llr[0, :, ::3] = 30.0  # a codeword whose waves are (partly) saturated from the first update on
    return llr


@pytest.mark.parametrize("name,B", CASES)
def test_first_decoder_constant_llr(name, B):
    big = B > 100
    with _forms(name, False) as (og, gg):
        sx, sz = _syndromes(og, B, 100)
        tx, tz = to_gpu(sx), to_gpu(sz)
        L0 = llr_const(0.05)
        for cn, factors in (("boxplus-phi", (1.0, 0.8)), ("boxplus", (0.8,)), ("minsum", (0.8,))):
            if big and cn != "boxplus-phi":
                continue
            for factor in factors:
                for iters in ((1, 3) if big else (0, 1, 2, 3)):
                    o = og.bp4_decode(sx, sz, iters, cn, factor, llr_const=L0, return_msgs=True)
                    for shortcut, fpe in MODES:
                        gg.set_saturation_shortcut(shortcut)
                        gg.set_fixed_point_exit(fpe)
                        g = gg.bp4_decode(tx, tz, iters, cn, factor, llr_const=L0, return_msgs=True)
                        _eq(o, g, f"{name} B={B} {cn} factor={factor} it={iters} shortcut={shortcut} exit={fpe}")


# (code, batch, launch): the register forms (NQ = 4 on [[882,24]], 5 on [[1270,28]]), the LDS form (two codewords per workgroup, a padded
# last workgroup; ibm72's default launch), the (4,4,8) kernels, and an irregular code on the runtime-degree path
LATER = [("ghp882", 3, None), ("ghp882", 257, None), ("ghp1270", 2, None), ("ghp882", 3, (256, 2)), ("ibm72", 77, None), ("gb48", 21, None),
         ("rsurf3", 9, None)]


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("name,B,launch", LATER)
def test_later_decoder_per_qubit_llrs(name, B, launch, shared):
    big = B > 100
    with _forms(name, shared) as (og, gg):
        if launch:
            gg.set_launch(*launch)
        sx, sz = _syndromes(og, B, 200)
        tx, tz = to_gpu(sx), to_gpu(sz)
        llr = _channel_llrs(B, gg.n, 11)
        tl = to_gpu(llr)
        for cn, factor in (("boxplus-phi", 1.0), ("boxplus-phi", 0.8), ("minsum", 0.8)):
            if big and (cn, factor) != ("boxplus-phi", 1.0):
                continue
            for iters in ((1, 3) if big else (0, 1, 2, 3)):
                o = og.bp4_decode(sx, sz, iters, cn, factor, llr_ch=llr, return_msgs=True)
                for shortcut, fpe in MODES:
                    gg.set_saturation_shortcut(shortcut)
                    gg.set_fixed_point_exit(fpe)
                    g = gg.bp4_decode(tx, tz, iters, cn, factor, llr_ch=tl, return_msgs=True)
                    _eq(o, g, f"{name} B={B} launch={launch} shared={shared} {cn} factor={factor} it={iters} shortcut={shortcut} exit={fpe}")


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("name,B", [("ghp882", 3), ("ghp1270", 2), ("ibm72", 77)])
def test_given_initial_messages_take_the_generic_path(name, B, shared):
    """msg_init given: non-zero arrays against the oracle, and all-zero arrays against the launch without them — the generic iteration 0
    and the closed / peeled one on the same device, byte for byte."""
    with _forms(name, shared) as (og, gg):
        sx, sz = _syndromes(og, B, 300)
        tx, tz = to_gpu(sx), to_gpu(sz)
        llr = _channel_llrs(B, gg.n, 12)
        rng = np.random.RandomState(5)
        init = (rng.uniform(-12, 12, size=(B, gg.E_x)).astype(np.float32), rng.uniform(-12, 12, size=(B, gg.E_z)).astype(np.float32))
        zeros = (np.zeros((B, gg.E_x), np.float32), np.zeros((B, gg.E_z), np.float32))
        L0 = llr_const(0.05)
        for chan_o, chan_g in ((dict(llr_const=L0), dict(llr_const=L0)), (dict(llr_ch=llr), dict(llr_ch=to_gpu(llr)))):
            for iters in (1, 2, 3):
                o_init = og.bp4_decode(sx, sz, iters, "boxplus-phi", 1.0, msg_init=init, return_msgs=True, **chan_o)
                o_zero = og.bp4_decode(sx, sz, iters, "boxplus-phi", 1.0, return_msgs=True, **chan_o)
                for shortcut, fpe in MODES:
                    gg.set_saturation_shortcut(shortcut)
                    gg.set_fixed_point_exit(fpe)
                    tag = f"{name} shared={shared} {sorted(chan_o)} it={iters} shortcut={shortcut} exit={fpe}"
                    g = gg.bp4_decode(tx, tz, iters, "boxplus-phi", 1.0, msg_init=tuple(to_gpu(a) for a in init), return_msgs=True, **chan_g)
                    _eq(o_init, g, tag + " msg_init")
                    g0 = gg.bp4_decode(tx, tz, iters, "boxplus-phi", 1.0, msg_init=tuple(to_gpu(a) for a in zeros), return_msgs=True, **chan_g)
                    g1 = gg.bp4_decode(tx, tz, iters, "boxplus-phi", 1.0, return_msgs=True, **chan_g)
                    _eq(o_zero, g0, tag + " msg_init = zeros")
                    _eq(g0, g1, tag + " zeros against none")


def test_trace_slot_zero_is_the_soft_syndrome_of_zero_messages():
    """Stage-two trace mode at num_iter = 2: slot 0 of the trace (and of the tape) is still taken from zero messages."""
    name, B, T = "ghp882", 3, 2
    with _forms(name, False) as (og, gg):
        sx, sz = _syndromes(og, B, 400)
        tx, tz = to_gpu(sx), to_gpu(sz)
        llr = _channel_llrs(B, gg.n, 13)
        L0 = llr_const(0.05)
        for chan_o, chan_g in ((dict(llr_const=L0), dict(llr_const=L0)), (dict(llr_ch=llr), dict(llr_ch=to_gpu(llr)))):
            tr = gg.bp4_decode_trace(tx, tz, T, "boxplus-phi", 1.0, want_tape=True, **chan_g)
            assert not tr["tape_x"][0].any().item() and not tr["tape_z"][0].any().item()
            for k in range(T + 1):
                o = og.bp4_decode(sx, sz, k, "boxplus-phi", 1.0, return_msgs=True, **chan_o)
                for key, got in (("x_logit", tr["x_logit"][k]), ("z_logit", tr["z_logit"][k]), ("msg_x", tr["tape_x"][k]),
                                 ("msg_z", tr["tape_z"][k])):
                    assert o[key].tobytes() == got.cpu().numpy().tobytes(), f"{sorted(chan_o)} trace slot {k} {key}"
            for key in ("llr", "x_hat", "z_hat"):
                assert o[key].tobytes() == tr[key].cpu().numpy().tobytes(), f"{sorted(chan_o)} trace {key}"


@pytest.mark.parametrize("compact", [False, True])
def test_sandwich_flags_with_short_decoders(compact):
    """Both forms inside the fused sandwich (first decoder closed form, later decoders peeled, 1 to 3 iterations each): the flags that
    send a codeword to the next round, the decisions and the marginals equal the oracle's."""
    from feedback_gnn_amd.graph import GnnWeights
    from feedback_gnn_amd.weights_io import read_weight_list
    name, B, iters = "ghp882", 5, [2, 1, 3]
    w = read_weight_list(WEIGHTS_882)
    with _forms(name, False) as (og, gg):
        ex, ez = og.pauli_noise(SEED, 0.10, 500, B)
        sx, sz = og.syndrome(ex, ez)
        gw = GnnWeights(w, gg.device)
        o = og.sandwich_decode(sx, sz, iters, [w] * 2, llr_const(0.05), return_llr=True)
        g = gg.sandwich_decode(to_gpu(sx), to_gpu(sz), iters, [gw] * 2, llr_const(0.05), compact=compact, return_llr=True, return_rounds=True)
    assert np.array_equal(o["rounds"], g["rounds"].cpu().numpy()) and o["rounds"].sum() > 0
    assert np.array_equal(o["x_hat"], g["x_hat"].cpu().numpy()) and np.array_equal(o["z_hat"], g["z_hat"].cpu().numpy())
    if not compact:
        assert o["llr"].tobytes() == g["llr"].cpu().numpy().tobytes()
