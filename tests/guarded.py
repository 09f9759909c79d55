"""A guarded, poisoned allocator for the buffers of a `TannerGraph` (a plain module: tests import it, pytest does not).

`guarded(graph)` replaces `graph._new` for the length of a `with` block.  Every buffer then is one uint8 tensor laid out as

    front guard (64 KiB of 0xA5) | payload (0xFF) | back guard (64 KiB of 0xA5)

and the tensor handed to the library is the payload viewed as the asked dtype and shape.  Two errors that a bit-exact comparison of a
fresh `torch.empty` cannot see become visible: a store beside the buffer changes a guard byte (`check`), and an element the kernel
never stores still holds the poison (`poison_left`: NaN as float32, 255 as uint8, -1 as int32 / int64) where a recycled block of
the caching allocator would still hold the previous kernel variant's correct values.  The guards see stores only: a read beside a
buffer returns 0xA5 bytes and nothing records it.
"""
import collections
import contextlib

import torch

GUARD_BYTES = 64 * 1024
GUARD_BYTE = 0xA5
POISON_BYTE = 0xFF
PAYLOAD_ALIGN = 256
assert GUARD_BYTES % PAYLOAD_ALIGN == 0  # the payload starts right behind the front guard

Record = collections.namedtuple("Record", "order shape dtype raw nbytes name")


class GuardError(AssertionError):
    pass


def _itemsize(dtype):
    return torch.empty(0, dtype=dtype).element_size()


class Guarded:
    def __init__(self, device):
        self.device = torch.device(device)
        self.records = []
        self.names = {}

    def alloc(self, shape, dtype, name=None):
        """A poisoned payload of `shape` / `dtype` between two guards, recorded.  Also the allocator for buffers a test hands in."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = _itemsize(dtype)
        count = 1
        for s in shape:
            count *= s
        slice_bytes = item
        for s in shape[1:]:
            slice_bytes *= s
        # a kernel that is off by one in the leading index (codeword b = B, trace slot k = T + 1) lands one slice beside the payload:
        # the guard has to hold all of it
        assert slice_bytes < GUARD_BYTES, (f"guard of {GUARD_BYTES} bytes does not cover one leading-dimension slice of {shape} {dtype} "
                                           f"({slice_bytes} bytes): use a smaller shape")
        nbytes = count * item
        raw = torch.empty(GUARD_BYTES + nbytes + GUARD_BYTES, dtype=torch.uint8, device=self.device)
        raw.fill_(GUARD_BYTE)
        raw[GUARD_BYTES:GUARD_BYTES + nbytes].fill_(POISON_BYTE)
        rec = Record(len(self.records), shape, dtype, raw, nbytes, name)
        self.records.append(rec)
        return self.payload(rec)

    @staticmethod
    def payload(rec):
        return rec.raw[GUARD_BYTES:GUARD_BYTES + rec.nbytes].view(rec.dtype).view(rec.shape)

    def record_of(self, t):
        """The record whose payload `t` is (or is a view into)."""
        p = t.data_ptr()
        for rec in self.records:
            lo = rec.raw.data_ptr() + GUARD_BYTES
            if rec.nbytes and lo <= p < lo + rec.nbytes:
                return rec
        raise KeyError("not a guarded tensor")

    def label(self, tensors):
        """Name the records behind the tensors of a result dict (None and empty entries are skipped): `check` then says which output."""
        for name, t in tensors.items():
            if isinstance(t, torch.Tensor) and t.numel():
                self.names[self.record_of(t).order] = name

    def check(self):
        """Synchronise once, then assert that both guards of every record still hold 0xA5 everywhere."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        for rec in self.records:
            front, back = rec.raw[:GUARD_BYTES], rec.raw[GUARD_BYTES + rec.nbytes:]
            changed = torch.cat([front != GUARD_BYTE, back != GUARD_BYTE])
            if not bool(changed.any()):
                continue
            idx = torch.nonzero(changed).flatten()
            # offsets relative to the payload: the front guard is [-GUARD_BYTES, 0), the back guard [nbytes, nbytes + GUARD_BYTES)
            off = [int(i) - GUARD_BYTES if int(i) < GUARD_BYTES else rec.nbytes + int(i) - GUARD_BYTES for i in (idx[0], idx[-1])]
            name = self.names.get(rec.order, rec.name)
            raise GuardError(f"write outside buffer #{rec.order}{'' if name is None else ' ' + repr(name)} shape {rec.shape} "
                             f"{rec.dtype} (payload {rec.nbytes} bytes): {int(idx.numel())} guard byte(s) changed, first at payload "
                             f"offset {off[0]}, last at payload offset {off[1]}")

    @staticmethod
    def poison_left(t):
        """How many elements of `t` still hold the poison pattern (every byte 0xFF)."""
        if t.numel() == 0:
            return 0
        b = t.contiguous().view(-1).view(torch.uint8).view(t.numel(), t.element_size())
        return int((b == POISON_BYTE).all(1).sum())

    @staticmethod
    def first_poison(t):
        """Flat index of the first element of `t` that still holds the poison, or None."""
        if t.numel() == 0:
            return None
        b = t.contiguous().view(-1).view(torch.uint8).view(t.numel(), t.element_size())
        idx = torch.nonzero((b == POISON_BYTE).all(1)).flatten()
        return int(idx[0]) if idx.numel() else None

    def assert_written(self, t, name):
        """Every element of the fully written output `t` was stored."""
        left = self.poison_left(t)
        assert left == 0, (f"{name} shape {tuple(t.shape)} {t.dtype}: {left} element(s) never written, the first at flat index "
                           f"{self.first_poison(t)}")

    def assert_untouched(self, t, name):
        """Every element of `t`, which the library is to leave alone, still holds the poison."""
        left = self.poison_left(t)
        assert left == t.numel(), f"{name} shape {tuple(t.shape)} {t.dtype}: {t.numel() - left} element(s) written that must be left alone"


@contextlib.contextmanager
def guarded(graph):
    """Replace `graph._new` on this instance by a guarded, poisoned allocator; the original is back afterwards, whatever happens.
    Yields the `Guarded` helper; `check()` runs once more on a clean exit."""
    helper = Guarded(graph.device)
    had = "_new" in vars(graph)
    saved = vars(graph).get("_new")
    graph._new = helper.alloc
    clean = False
    try:
        yield helper
        clean = True
    finally:
        if had:
            graph._new = saved
        else:
            del graph._new
    if clean:
        helper.check()
