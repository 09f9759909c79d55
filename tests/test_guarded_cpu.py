"""The guarded allocator of tests/guarded.py detects what it is there to detect, shown on CPU tensors: a byte stored anywhere in
either guard fails `check()` with the record and the offset, an element never stored is counted, `_new` comes back after an exception,
and a shape whose leading-dimension slice the guard cannot hold is refused.  The last test reads the source of `TannerGraph`: the guard
reaches only what goes through `_new`, so nothing in the class may allocate beside it."""
import pytest
import torch

from guarded import GUARD_BYTE, GUARD_BYTES, PAYLOAD_ALIGN, POISON_BYTE, GuardError, Guarded, guarded


class _Stub:
    device = torch.device("cpu")

    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)


def test_layout_fill_and_view():
    g = _Stub()
    with guarded(g) as h:
        t = g._new((3, 5), torch.float32)
        u = h.alloc((7,), torch.uint8, name="errors")
        i32, i64 = g._new((4,), torch.int32), h.alloc((2, 3), torch.int64)
        empty = g._new((0, 3, 7), torch.float32)
        assert [r.order for r in h.records] == [0, 1, 2, 3, 4] and h.records[1].name == "errors"
        assert [(r.shape, r.dtype) for r in h.records[:2]] == [((3, 5), torch.float32), ((7,), torch.uint8)]
        for r, want in zip(h.records, (60, 7, 16, 48, 0)):
            assert r.raw.dtype == torch.uint8 and r.raw.numel() == 2 * GUARD_BYTES + want and r.nbytes == want
            assert bool((r.raw[:GUARD_BYTES] == GUARD_BYTE).all()) and bool((r.raw[GUARD_BYTES + want:] == GUARD_BYTE).all())
            assert bool((r.raw[GUARD_BYTES:GUARD_BYTES + want] == POISON_BYTE).all())
        for x, r in zip((t, u, i32, i64), h.records):
            assert x.is_contiguous() and x.device == g.device
            assert x.data_ptr() == r.raw.data_ptr() + GUARD_BYTES and (x.data_ptr() - r.raw.data_ptr()) % PAYLOAD_ALIGN == 0
            assert h.record_of(x) is r
        assert t.shape == (3, 5) and bool(torch.isnan(t).all())
        assert bool((u == 255).all()) and bool((i32 == -1).all()) and bool((i64 == -1).all())
        assert empty.shape == (0, 3, 7) and empty.dtype == torch.float32 and h.poison_left(empty) == 0
        h.check()


@pytest.mark.parametrize("dtype,shape", [(torch.uint8, (5, 7)), (torch.float32, (3, 3, 7)), (torch.int32, (0, 4))])
@pytest.mark.parametrize("where", ["end", "end+65535", "start-1", "start-65536"])
def test_one_byte_outside_the_payload_fails_the_check(where, dtype, shape):
    g = _Stub()
    h = Guarded(g.device)
    h.alloc((4,), torch.float32)
    t = h.alloc(shape, dtype, name="victim")
    h.alloc((9,), torch.uint8)
    rec = h.records[1]
    nbytes = t.numel() * t.element_size()
    off = {"end": nbytes, "end+65535": nbytes + 65535, "start-1": -1, "start-65536": -65536}[where]
    h.check()
    rec.raw[GUARD_BYTES + off] = 0  # through the raw tensor: the payload view cannot reach it
    with pytest.raises(GuardError) as err:
        h.check()
    msg = str(err.value)
    assert "#1 'victim'" in msg and str(shape) in msg and str(dtype) in msg
    assert f"first at payload offset {off}, last at payload offset {off}" in msg and "1 guard byte(s)" in msg
    rec.raw[GUARD_BYTES + off] = GUARD_BYTE
    h.check()


def test_first_and_last_changed_offsets_are_reported():
    h = Guarded("cpu")
    h.alloc((10,), torch.uint8)
    raw = h.records[0].raw
    raw[GUARD_BYTES - 3] = 1
    raw[GUARD_BYTES + 10 + 4] = 1
    raw[GUARD_BYTES + 10 + 100] = 1
    with pytest.raises(GuardError, match=r"3 guard byte\(s\) changed, first at payload offset -3, last at payload offset 110"):
        h.check()


def test_a_guard_byte_value_written_into_the_payload_is_no_guard_failure():
    h = Guarded("cpu")
    t = h.alloc((6,), torch.uint8)
    t.fill_(GUARD_BYTE)
    t[0], t[5] = 0, 0
    h.check()


def test_the_check_runs_on_leaving_the_context():
    g = _Stub()
    with pytest.raises(GuardError, match="payload offset 12"):
        with guarded(g) as h:
            g._new((3,), torch.float32)
            h.records[0].raw[GUARD_BYTES + 12] = 7


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64, torch.float32])
def test_poison_left_counts_the_unwritten_elements(dtype):
    h = Guarded("cpu")
    t = h.alloc((4, 5), dtype)
    assert h.poison_left(t) == 20 and h.first_poison(t) == 0
    h.assert_untouched(t, "t")
    t[:, :4] = 1
    t[0, 4] = 0
    assert h.poison_left(t) == 3 and h.first_poison(t) == 9 and h.poison_left(t[:1]) == 0 and h.poison_left(t[1:]) == 3
    with pytest.raises(AssertionError, match="3 element.* never written, the first at flat index 9"):
        h.assert_written(t, "t")
    with pytest.raises(AssertionError, match="17 element.* written that must be left alone"):
        h.assert_untouched(t, "t")
    t[1:, 4] = 2
    assert h.poison_left(t) == 0 and h.first_poison(t) is None
    h.assert_written(t, "t")
    if dtype != torch.uint8:  # one byte of an element stored: it is no poison any more
        u = h.alloc((3,), dtype)
        h.record_of(u).raw[GUARD_BYTES + u.element_size()] = 0
        assert h.poison_left(u) == 2


def test_new_is_restored_after_an_exception():
    g = _Stub()
    before = g._new
    assert "_new" not in vars(g)
    with pytest.raises(RuntimeError, match="boom"):
        with guarded(g) as h:
            assert g._new == h.alloc
            raise RuntimeError("boom")
    assert "_new" not in vars(g) and g._new == before and g._new((2,), torch.uint8).shape == (2,)
    own = lambda shape, dtype: torch.zeros(shape, dtype=dtype)  # noqa: E731 -- an instance that already carries its own _new
    g._new = own
    with pytest.raises(RuntimeError):
        with guarded(g):
            raise RuntimeError("boom")
    assert g._new is own


def test_an_exception_inside_the_context_is_not_replaced_by_the_guard_failure():
    g = _Stub()
    with pytest.raises(RuntimeError, match="boom"):
        with guarded(g) as h:
            g._new((3,), torch.float32)
            h.records[0].raw[0] = 0
            raise RuntimeError("boom")


def test_the_guard_must_hold_one_leading_dimension_slice():
    h = Guarded("cpu")
    h.alloc((2, GUARD_BYTES // 4 - 1), torch.float32)  # 65 532 bytes per slice
    h.alloc((GUARD_BYTES * 4,), torch.uint8)  # a flat workspace: one byte per slice, any length
    with pytest.raises(AssertionError, match="does not cover one leading-dimension slice"):
        h.alloc((2, GUARD_BYTES // 4), torch.float32)
    with pytest.raises(AssertionError, match="does not cover one leading-dimension slice"):
        h.alloc((3, 4, GUARD_BYTES // 4), torch.uint8)
    assert len(h.records) == 2


def test_no_tanner_graph_method_allocates_beside_new():
    """Every output and workspace of the class goes through `_new`: its body names torch's allocators once, in `_new` itself."""
    import inspect
    import re
    from feedback_gnn_amd.graph import TannerGraph
    src = inspect.getsource(TannerGraph)
    hits = [line.strip() for line in src.splitlines() if re.search(r"torch\.(empty|zeros|ones|full|rand|randn|tensor|arange)\w*\(", line)]
    assert hits == ["return torch.empty(shape, dtype=dtype, device=self.device)"], hits
