"""Self-test of tests/guarded_buffers.py: a clean run passes, and one byte written into a leading guard, into a trailing
guard and into an input is each reported with the buffer's name and the offset in rows.  The host part needs no GPU; the
`gpu` part does the same with a tensor indexing write into the device arena (an ordinary tensor operation on memory the
test owns)."""
import re
import numpy as np
import pytest

import guarded_buffers as gb

ROW, RPS, STREAMS = 96, 3, 5                                # rows of 96 bytes, 3 per stream, 5 streams


def _arena(device):
    n = STREAMS * RPS * ROW
    a = gb.build(device, [
        dict(name="d_in", nbytes=n, align=16, role="in", guard=STREAMS * 5 * ROW, row=ROW, rows_per_stream=RPS),
        dict(name="d_out", nbytes=n, align=8, role="out", guard=STREAMS * 5 * ROW, row=ROW, rows_per_stream=RPS),
        dict(name="d_bits", nbytes=4 * STREAMS * RPS, align=4, role="out", row=4, rows_per_stream=RPS),
        dict(name="d_bytes", nbytes=77, align=1, role="inout"),
    ])
    a.load("d_in", np.arange(n, dtype=np.uint8))
    a.load("d_bytes", np.full(77, 0xA5, np.uint8))
    return a


def _poke(a, name, rel, value=None):
    """One byte at rel bytes from the region's start (negative: the leading guard), changed to value (default: its complement)."""
    off = a.regions[name].off + rel
    if a.t is None:
        a.np[off] = (~a.np[off]) if value is None else value
    else:
        a.t[off] = (~a.t[off]) if value is None else value


def _layout_ok(a):
    for r in a.regions.values():
        addr = a.base + r.off
        assert addr % r.align == 0 and (addr // r.align) % 2 == 1, f"{r.name} must start at an odd multiple of {r.align}"
        assert r.guard >= gb.MIN_GUARD
    regs = sorted(a.regions.values(), key=lambda r: r.off)
    for p, q in zip(regs, regs[1:]):
        assert p.off + p.nbytes + p.guard <= q.off - q.guard, "guards of neighbouring regions must not overlap"


def _self_test(device):
    a = _arena(device)
    _layout_ok(a)
    a.check({"d_out": STREAMS * RPS * ROW})                 # clean: passes
    # an output may be written anywhere inside its region, and an inout too
    _poke(a, "d_out", 0); _poke(a, "d_out", STREAMS * RPS * ROW - 1); _poke(a, "d_bytes", 5)
    a.check()
    n = STREAMS * RPS * ROW
    cases = [
        # (buffer, byte relative to the region, what the report must say)
        ("d_out", -1, r"leading guard of d_out written: 1 bytes, first at byte -1 = row -1 \(stream -1, block 2, byte 95\)"),
        ("d_out", n, rf"trailing guard of d_out written: 1 bytes, first at byte {n} = row 15 \(stream 5, block 0, byte 0\)"),
        ("d_out", n + 2 * ROW + 7, rf"trailing guard of d_out written: 1 bytes, first at byte {n + 2 * ROW + 7} = row 17 \(stream 5, block 2, byte 7\)"),
        ("d_in", 7 * ROW + 11, rf"input d_in modified: 1 bytes, first at byte {7 * ROW + 11} = row 7 \(stream 2, block 1, byte 11\)"),
        ("d_bits", -4, r"leading guard of d_bits written: 1 bytes, first at byte -4 = row -1 \(stream -1, block 2, byte 0\)"),
        ("d_bits", 4 * STREAMS * RPS + gb.MIN_GUARD - 1, r"trailing guard of d_bits written"),
    ]
    for name, rel, want in cases:
        a = _arena(device)
        _poke(a, name, rel)
        with pytest.raises(gb.GuardError) as e:
            a.check()
        msg = str(e.value)
        assert re.search(want, msg), f"{name} @ {rel}: report was {msg!r}"
        others = [o for o in a.regions if o != name and re.search(rf"\b{o}\b", msg)]
        assert not others, f"{name} @ {rel}: the report also names {others}: {msg!r}"
    # zeros, 0xFF and a copied row are all visible: the pattern is not constant and no two rows agree
    for fill in (0x00, 0xFF):
        a = _arena(device)
        r = a.regions["d_out"]
        lo = r.off + r.nbytes
        if a.t is None: a.np[lo:lo + ROW] = fill
        else: a.t[lo:lo + ROW] = fill
        with pytest.raises(gb.GuardError, match=r"trailing guard of d_out written: 9[0-9] bytes"):
            a.check()
    a = _arena(device)
    r = a.regions["d_out"]
    lo = r.off + r.nbytes
    if a.t is None: a.np[lo:lo + ROW] = a.np[lo - ROW:lo].copy()
    else: a.t[lo:lo + ROW] = a.t[lo - ROW:lo].clone()
    with pytest.raises(gb.GuardError, match=r"trailing guard of d_out written"):
        a.check()
    # both directions: first and last offending byte
    a = _arena(device)
    _poke(a, "d_in", 3); _poke(a, "d_in", n - 2)
    with pytest.raises(gb.GuardError, match=rf"input d_in modified: 2 bytes, first at byte 3 = row 0 .*, last at byte {n - 2} = row 14 \(stream 4, block 2, byte 94\)"):
        a.check()
    # repoison: an input given back to the pattern counts as loaded with it
    a = _arena(device)
    a.repoison("d_in", a.poison_of("d_in"))
    a.check()
    assert np.array_equal(a.fetch("d_in"), gb.pattern(a.regions["d_in"].off, n))
    _poke(a, "d_in", 40)
    with pytest.raises(gb.GuardError, match=r"input d_in modified: 1 bytes, first at byte 40 "):
        a.check()


def test_pattern_is_position_dependent():
    p = gb.pattern(0, 4096)
    assert (p[1:] != p[:-1]).all() and len(set(p[:256].tolist())) == 256
    for row in (16, 96, 256, 512, 4096 + 16, 16384, 65536, 1 << 20):   # a row copied over its neighbour differs in (nearly) every byte
        q = gb.pattern(12345, 2 * row)
        assert (q[:row] != q[row:]).mean() > 0.99, row


def test_host_arena_reports_each_violation_with_name_and_offset():
    _self_test(None)


@pytest.mark.gpu
def test_device_arena_reports_each_violation_with_name_and_offset():
    import torch
    _self_test(torch.device("cuda", 0))
    torch.cuda.synchronize()
