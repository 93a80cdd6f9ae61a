"""Guard-band placement of tensors: does a kernel stay inside the buffers it was given?

Every parity test hands the kernels tensors that torch allocated fresh: the base is 256-B
aligned, the block is rounded up, and nothing the test owns lies before or after it.  A store a
few bytes outside the destination, an element never written (the caching allocator returns the
block the previous call of the same shape just freed, still holding the right answer) and a
result that depends on the buffer's alignment are invisible there.  This module puts a tensor
INSIDE a larger allocation instead:

    arena(shape, dtype, device, offset_elems)  ->  (view, arena)

      arena:  [ guard | offset | view ............ | guard ]      one flat tensor, every byte
                                                                  a sentinel

The sentinel is a quiet NaN with a recognisable payload for floating dtypes and 0xA5 bytes for
integer dtypes.  guards_intact(arena, view) compares everything outside the view with the
sentinel byte for byte; sentinel_count(t) counts result elements that still hold it (never
written); and because the guards are NaN, an out-of-range read that reaches the arithmetic,
even with weight 0, shows up as a NaN in the result (reads that are clamped or range-checked do
not).  placed(monkeypatch, offset_elems) routes the allocations the package makes for its
results (torch.empty / empty_like / zeros / zeros_like) through arena() and checks every guard
when it exits.

Offsets are whole elements, so a base is never less aligned than its element size (the float
atomics of the backward kernels stay naturally aligned), and view and guards are one valid
allocation: a kernel that overruns damages only sentinel bytes the test owns.

Not a conftest and not a test: imported like tests/fused_variants.py."""
import contextlib

import torch

# the real allocators, whatever placed() patches into the torch namespace meanwhile
_EMPTY, _EMPTY_LIKE, _ZEROS, _ZEROS_LIKE = torch.empty, torch.empty_like, torch.zeros, torch.zeros_like

GUARD_BYTES = 4096          # at least this much sentinel on each side of a view ...
GUARD_ROWS = 2              # ... and at least this many rows of the tensor ...
GUARD_WINDOW = 256          # ... plus one column window of the streaming kernels
BASE_ALIGN = 256            # what torch's allocator gives: offset 0 keeps the view this aligned

# quiet NaNs with payload 1 (bf16 0x7FC1, f16 0x7E01, f32 0x7FC00001, f64 likewise)
_FLOAT_SENTINEL = {
    torch.bfloat16: (torch.int16, 0x7FC1),
    torch.float16: (torch.int16, 0x7E01),
    torch.float32: (torch.int32, 0x7FC00001),
    torch.float64: (torch.int64, 0x7FF8000000000001),
}
INT_SENTINEL_BYTE = 0xA5


def sentinel_bytes(dtype):
    """The sentinel of one element of dtype as little-endian bytes."""
    es = _EMPTY((), dtype=dtype).element_size()
    if dtype in _FLOAT_SENTINEL:
        return list(_FLOAT_SENTINEL[dtype][1].to_bytes(es, "little"))
    return [INT_SENTINEL_BYTE] * es


def _fill_sentinel(flat):
    if flat.dtype in _FLOAT_SENTINEL:
        idt, bits = _FLOAT_SENTINEL[flat.dtype]
        flat.view(idt).fill_(bits)
    else:
        flat.view(torch.uint8).fill_(INT_SENTINEL_BYTE)


def default_guard_elems(shape, dtype):
    """Elements of sentinel on each side: >= 4 KiB, >= two rows plus a 256-column window (an
    overrun of one whole row and a window still lands inside), rounded up so that the guard is
    a whole number of 256-B blocks (offset 0 then leaves the view as aligned as a fresh
    allocation)."""
    es = _EMPTY((), dtype=dtype).element_size()
    row = int(shape[-1]) if len(shape) else 1
    n = max(-(-GUARD_BYTES // es), GUARD_ROWS * row + GUARD_WINDOW)
    per = BASE_ALIGN // es
    return -(-n // per) * per


def arena(shape, dtype, device="cpu", offset_elems=0, guard_elems=None, fill=None):
    """(view, arena): a contiguous `shape` view that starts guard_elems + offset_elems elements
    into one flat sentinel-filled tensor, with at least guard_elems elements after it.  fill:
    None leaves the sentinel in the view too (an element the kernel never writes then shows in
    the result); a number fills the view with it (torch.zeros)."""
    shape = tuple(int(s) for s in shape)
    numel = 1
    for s in shape:
        numel *= s
    floor = default_guard_elems(shape, dtype)
    guard = floor if guard_elems is None else int(guard_elems)
    if guard < floor:
        raise ValueError(f"guard of {guard} elements is below the floor {floor} for {shape} {dtype}")
    offset_elems = int(offset_elems)
    if offset_elems < 0:
        raise ValueError("offset_elems must be a whole, non-negative number of elements")
    flat = _EMPTY(guard + offset_elems + numel + guard, dtype=dtype, device=device)
    _fill_sentinel(flat)
    start = guard + offset_elems
    view = flat[start:start + numel].view(shape)
    if fill is not None:
        view.fill_(fill)
    return view, flat


def _span(arena_t, view):
    """Byte range [b0, b1) of the view inside its arena."""
    es = arena_t.element_size()
    b0 = view.data_ptr() - arena_t.data_ptr()
    b1 = b0 + view.numel() * es
    total = arena_t.numel() * es
    assert view.is_contiguous() and view.dtype == arena_t.dtype
    assert 0 <= b0 <= b1 <= total, "the view does not lie inside the arena"
    return b0, b1, total


def guard_gaps(arena_t, view):
    """Bytes of sentinel before and after the view."""
    b0, b1, total = _span(arena_t, view)
    return b0, total - b1


def guards_intact(arena_t, view, what=""):
    """Every byte of the arena outside the view still holds the sentinel (compared as raw
    bytes); else AssertionError naming the first and last damaged byte relative to the view's
    ends: -k is k bytes before element 0, +k is k bytes after the last element's last byte
    (+0 the first byte past the end)."""
    b0, b1, total = _span(arena_t, view)
    es = arena_t.element_size()
    raw = arena_t.view(torch.uint8)
    pat = torch.tensor(sentinel_bytes(arena_t.dtype), dtype=torch.uint8, device=raw.device)
    bad = (raw.view(-1, es) != pat[None, :]).view(-1)
    msgs = []
    lead = torch.nonzero(bad[:b0]).view(-1)
    if lead.numel():
        msgs.append(f"{lead.numel()} guard bytes damaged before the view: first at "
                    f"{int(lead[0]) - b0}, last at {int(lead[-1]) - b0} (bytes from element 0)")
    trail = torch.nonzero(bad[b1:]).view(-1)
    if trail.numel():
        msgs.append(f"{trail.numel()} guard bytes damaged after the view: first at "
                    f"+{int(trail[0])}, last at +{int(trail[-1])} (bytes past the end)")
    assert not msgs, f"{what}{tuple(view.shape)} {view.dtype}: " + "; ".join(msgs)
    return True


def sentinel_mask(t):
    """Boolean mask of the elements of t whose bits are exactly the sentinel's."""
    t = t.contiguous()
    if t.dtype in _FLOAT_SENTINEL:
        idt, bits = _FLOAT_SENTINEL[t.dtype]
        return t.view(idt) == bits
    es = t.element_size()
    return (t.view(torch.uint8).view(-1, es) == INT_SENTINEL_BYTE).all(dim=1).view(t.shape)


def sentinel_count(t):
    """How many elements of t were never written (still hold the sentinel)."""
    return int(sentinel_mask(t).sum().item())


def place(t, device=None, offset_elems=0):
    """A copy of t inside a fresh arena on device: (view, arena)."""
    device = t.device if device is None else device
    view, flat = arena(tuple(t.shape), t.dtype, device, offset_elems)
    view.copy_(t)
    return view, flat


class Placement:
    """What placed() handed out: (arena, view) pairs, in allocation order."""

    def __init__(self):
        self.arenas = []

    def add(self, arena_t, view):
        self.arenas.append((arena_t, view))

    def check(self, what=""):
        for a, v in self.arenas:
            guards_intact(a, v, what)

    def arena_of(self, t):
        """The (arena, view) whose view starts where t does, or None."""
        for a, v in self.arenas:
            if v.data_ptr() == t.data_ptr() and v.dtype == t.dtype:
                return a, v
        return None


def _size_arg(args):
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(s) for s in args[0])
    if args and all(isinstance(a, int) for a in args):
        return tuple(args)
    return None


@contextlib.contextmanager
def placed(monkeypatch, offset_elems=0, device_types=("cuda",), min_dim=2):
    """Route the package's result allocations through arena() for the duration of the block.

    torch.empty, torch.empty_like, torch.zeros and torch.zeros_like are what HyGrid/ops.py,
    HexFrames.py and pipeline.py allocate with; a call for a tensor of min_dim or more
    dimensions on one of device_types gets an arena view (sentinel-filled for empty, zero for
    zeros), everything else, and any call with arguments beyond size / dtype / device, passes
    through to torch.  offset_elems: an int, or a function (dtype, ndim) -> elements.

    Yields the Placement that records every arena handed out; when the block ends without an
    exception the device is synchronised and guards_intact runs on each of them."""
    rec = Placement()

    def offset_for(dtype, ndim):
        return int(offset_elems(dtype, ndim)) if callable(offset_elems) else int(offset_elems)

    def route(shape, dtype, device, fill):
        if shape is None or dtype is None or device is None:
            return None
        device = torch.device(device)
        if device.type not in device_types or len(shape) < min_dim:
            return None
        if any(s <= 0 for s in shape):
            return None
        view, flat = arena(shape, dtype, device, offset_for(dtype, len(shape)), fill=fill)
        rec.add(flat, view)
        return view

    def make(real, fill):
        def alloc(*args, **kw):
            if set(kw) <= {"dtype", "device"}:
                out = route(_size_arg(args), kw.get("dtype") or torch.get_default_dtype(),
                            kw.get("device") or "cpu", fill)
                if out is not None:
                    return out
            return real(*args, **kw)
        return alloc

    def make_like(real, fill):
        def alloc_like(t, **kw):
            if set(kw) <= {"dtype", "device"} and t.is_contiguous():
                out = route(tuple(t.shape), kw.get("dtype") or t.dtype,
                            kw.get("device") or t.device, fill)
                if out is not None:
                    return out
            return real(t, **kw)
        return alloc_like

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", make(_EMPTY, None))
        m.setattr(torch, "zeros", make(_ZEROS, 0))
        m.setattr(torch, "empty_like", make_like(_EMPTY_LIKE, None))
        m.setattr(torch, "zeros_like", make_like(_ZEROS_LIKE, 0))
        yield rec
    if "cuda" in device_types and torch.cuda.is_available():
        torch.cuda.synchronize()
    rec.check()
