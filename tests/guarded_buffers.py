"""Poisoned, guarded caller buffers for the entry points of include/ulc_amd.h ("Caller buffers" there).

An Arena is ONE allocation - a numpy array for the host forms, a torch.uint8 tensor for the device forms - filled with a
position-dependent byte pattern.  carve() hands out regions inside it: each starts at an ODD multiple of the alignment the
header states (so no call passes thanks to more alignment than the contract gives) and sits between two guards of the
caller's size, never less than 4 KiB.  The tests size a guard as the buffer would be at maxBlocksPerCall blocks: a store one
block, one stream or "indexed by maxBlocksPerCall" too far lands in a guard, in memory the test owns.  check() then asserts
that every guard byte still holds the pattern and that every input still holds what was loaded, and names the buffer and
the row (stream, block, byte) of the first and of the last byte that does not.

The pattern is position dependent and never constant over a row: a kernel that writes zeros, 0xFF or a copy of the row
beside it changes bytes.  (A store that happens to write the pattern's own byte is not seen: one in 256 per byte.)"""
import numpy as np

MIN_GUARD = 4096
ROLES = ("in", "out", "inout")


def pattern(start, n):
    """Bytes start .. start + n - 1 of the poison: (i * 167 + 13) & 0xFF with the higher bytes of i mixed in.  The plain form
    has period 256, and the rows of a PCM buffer are multiples of 256 bytes: a row copied over its neighbour would not show.
    No two neighbours agree (the steps are 167, 258, 315 and 346 mod 256), and two positions a multiple of 256 apart agree
    only when they are 2^32 apart."""
    # i = 256 j + l: the byte is (167 l) + (13 + 91 j + 57 (j >> 8) + 31 (j >> 16)) mod 256, formed per group of 256 bytes
    lo = start & ~255
    j = np.arange(lo >> 8, (start + n + 255) >> 8, dtype=np.int64)
    base = ((13 + j * 91 + (j >> 8) * 57 + (j >> 16) * 31) & 0xFF).astype(np.uint8)
    low = ((np.arange(256) * 167) & 0xFF).astype(np.uint8)
    return (base[:, None] + low[None, :]).reshape(-1)[start - lo:start - lo + n]      # (uint8 sums wrap)


class GuardError(AssertionError):
    pass


class _Region:
    def __init__(self, name, off, nbytes, align, role, guard, row, rows_per_stream):
        self.name, self.off, self.nbytes, self.align, self.role, self.guard = name, off, nbytes, align, role, guard
        self.row, self.rows_per_stream = row, rows_per_stream
        self.loaded = None                                 # what load() wrote (bytes), for the roles that have an input


def footprint(nbytes, align, guard):
    """Most bytes of an arena one region can take: two guards, the region, and the slack of placing it on an odd multiple."""
    return 2 * max(int(guard), MIN_GUARD) + int(nbytes) + 2 * max(int(align), 1)


class Arena:
    """capacity bytes of poison; device None: host memory (numpy), else a torch device."""

    def __init__(self, capacity, device=None):
        self.capacity = int(capacity)
        self.device = device
        if device is None:
            self.np = pattern(0, self.capacity)
            self.t = None
            self.base = self.np.ctypes.data
        else:
            import torch
            self.t = torch.from_numpy(pattern(0, self.capacity)).to(device)
            self.np = None
            self.base = self.t.data_ptr()
        self.cursor = 0
        self.regions = {}

    # ---- layout ----------------------------------------------------------------------------------------------------
    def carve(self, name, nbytes, align, role, guard=0, row=None, rows_per_stream=1):
        """-> address of a region of nbytes.  align: what the header states for this pointer (1: none); role: in / out / inout;
        guard: bytes of the guard on either side (at least 4 KiB); row, rows_per_stream: bytes of one row of the buffer and rows
        per stream, so that a report can name (stream, block, byte)."""
        assert role in ROLES and name not in self.regions and nbytes > 0
        align, guard = max(int(align), 1), max(int(guard), MIN_GUARD)
        addr = self.base + self.cursor + guard
        q = -(-addr // align)                              # first multiple of align at or behind the leading guard ...
        if q % 2 == 0:
            q += 1                                         # ... that is an odd one
        off = q * align - self.base
        assert off + nbytes + guard <= self.capacity, f"arena of {self.capacity} bytes too small for {name}"
        self.regions[name] = _Region(name, off, int(nbytes), align, role, guard, int(row or nbytes), int(rows_per_stream))
        self.cursor = off + nbytes + guard
        assert (self.base + off) % align == 0 and ((self.base + off) // align) % 2 == 1
        return self.base + off

    def ptr(self, name):
        return self.base + self.regions[name].off

    def view(self, name, dtype=np.uint8):
        """The region as a tensor (device arena) or array (host arena) of dtype, aliasing the arena."""
        r = self.regions[name]
        if self.t is None:
            return self.np[r.off:r.off + r.nbytes].view(dtype)
        import torch
        td = getattr(torch, np.dtype(dtype).name)
        return self.t[r.off:r.off + r.nbytes].view(td)

    def load(self, name, array):
        """Contents of an `in` or `inout` region (exactly its size)."""
        r = self.regions[name]
        assert r.role in ("in", "inout"), f"{name} is an output"
        b = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert b.size == r.nbytes, f"{name}: {b.size} bytes loaded into a region of {r.nbytes}"
        r.loaded = b.copy()
        if self.t is None:
            self.np[r.off:r.off + r.nbytes] = b
        else:
            import torch
            self.t[r.off:r.off + r.nbytes] = torch.from_numpy(r.loaded).to(self.device)

    def expect(self, name, array):
        """What an input region holds when the caller wrote it through view() itself (a copy on a stream)."""
        r = self.regions[name]
        b = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        assert r.role in ("in", "inout") and b.size == r.nbytes
        r.loaded = b.copy()

    def poison_of(self, name):
        """The pattern's bytes for the region, in memory of the arena's kind (a source for repoison() made ahead of time)."""
        r = self.regions[name]
        p = pattern(r.off, r.nbytes)
        if self.t is None:
            return p
        import torch
        return torch.from_numpy(p).to(self.device)

    def repoison(self, name, src=None):
        """The region back to the pattern.  Device arena: a device-to-device copy on the current stream when src (poison_of)
        is given, so that nothing waits for the host.  An input then counts as loaded with the pattern."""
        r = self.regions[name]
        src = self.poison_of(name) if src is None else src
        if self.t is None:
            self.np[r.off:r.off + r.nbytes] = src
        else:
            self.t[r.off:r.off + r.nbytes].copy_(src, non_blocking=True)
        r.loaded = pattern(r.off, r.nbytes)

    def fetch(self, name, dtype=np.uint8):
        """Host copy of the region's bytes as dtype (after the caller synchronised)."""
        r = self.regions[name]
        if self.t is None:
            return self.np[r.off:r.off + r.nbytes].copy().view(dtype)
        return self.t[r.off:r.off + r.nbytes].cpu().numpy().view(dtype)

    # ---- the check -------------------------------------------------------------------------------------------------
    @staticmethod
    def _where(r, i):
        """Byte i relative to the region's start (negative: in front of it) in rows of the buffer."""
        row, rel = i // r.row, i % r.row
        return f"byte {i} = row {row} (stream {row // r.rows_per_stream}, block {row % r.rows_per_stream}, byte {rel})"

    def check(self, defined=None):
        """After synchronisation: (a) every guard byte holds the pattern, (b) every `in` region equals what was loaded,
        (c) nothing is asserted here about `out` regions: their defined extents are the caller's to compare (defined maps a
        name to a boolean byte mask or a byte count and is only validated against the region's size; the bytes of an output
        outside it may hold anything).  Raises GuardError naming the buffer and the first and last offending byte."""
        host = self.np if self.t is None else self.t.cpu().numpy()
        for name, d in (defined or {}).items():
            r = self.regions[name]
            assert r.role != "in", f"{name} is an input: all of it is checked"
            n = int(d) if np.isscalar(d) else np.asarray(d).size
            assert 0 <= n <= r.nbytes, f"defined extent of {name} exceeds the region"
        errors = []
        for r in self.regions.values():
            for side, lo in (("leading", r.off - r.guard), ("trailing", r.off + r.nbytes)):
                bad = np.flatnonzero(host[lo:lo + r.guard] != pattern(lo, r.guard))
                if bad.size:
                    first, last = lo + int(bad[0]) - r.off, lo + int(bad[-1]) - r.off
                    errors.append(f"{side} guard of {r.name} written: {bad.size} bytes, first at {self._where(r, first)}, "
                                  f"last at {self._where(r, last)} (region: {r.nbytes} bytes, rows of {r.row})")
            if r.role == "in":
                assert r.loaded is not None, f"input {r.name} was never loaded"
                bad = np.flatnonzero(host[r.off:r.off + r.nbytes] != r.loaded)
                if bad.size:
                    errors.append(f"input {r.name} modified: {bad.size} bytes, first at {self._where(r, int(bad[0]))}, "
                                  f"last at {self._where(r, int(bad[-1]))}")
        # the bytes between the regions' guards (placement slack) belong to nobody
        owned = np.zeros(self.capacity, bool)
        for r in self.regions.values():
            owned[r.off - r.guard:r.off + r.nbytes + r.guard] = True
        free = np.flatnonzero(~owned)
        if free.size:
            bad = free[host[free] != pattern(0, self.capacity)[free]]
            if bad.size:
                errors.append(f"arena bytes outside every region and guard written: {bad.size}, first at arena offset {int(bad[0])}")
        if errors:
            raise GuardError("; ".join(errors))


def build(device, specs):
    """Arena for a list of carve() keyword dicts (name, nbytes, align, role[, guard, row, rows_per_stream]), all carved."""
    cap = sum(footprint(s["nbytes"], s.get("align", 1), s.get("guard", 0)) for s in specs) + 64
    a = Arena(cap, device)
    for s in specs:
        a.carve(**s)
    return a
