"""The call axis on the GPU: every call family behind every call family on one encoder and one decoder object per geometry
(tests/call_axis_testlib.py; the census of the sequences is tests/test_call_axis_capi.py's).  Every output of every call is
compared bit for bit with the oracle's model of the object; the library is compared with itself only where the property is an
identity - a call that leaves stream state alone leaves save_streams of all slots byte for byte unchanged.

  1. one call at a time, synchronised: a failure names the call, the pair of families and whether the call was the family's first
  2. the ORDER contract (include/ulc_amd.h): the same calls without the host forms, enqueued on one stream behind filler work
     that keeps the device busy until the first call has returned, nothing synchronised until the end; run twice on one object
  3. the sequences of two pairs of objects of different geometry interleaved call by call on one stream"""
import math
import os
import time
import numpy as np
import pytest

import call_axis_testlib as A

pytestmark = pytest.mark.gpu
CASES = [(kind, name, start) for kind in ("dec", "enc") for name in A.GEOMS[kind] for start in A.STARTS]
ids = lambda c: "-".join(c)
MARGIN = 4                                                  # the filler runs this many times as long as the first call takes to return


def _note(line):
    """a figure for profiles/call_axis_evidence.txt: printed, and appended to the file CALL_AXIS_EVIDENCE names"""
    print(line)
    if os.environ.get("CALL_AXIS_EVIDENCE"):
        with open(os.environ["CALL_AXIS_EVIDENCE"], "a") as f:
            f.write(line + "\n")


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sequence_synchronised(case):
    kind, name, start = case
    seq = A.sequence(kind, name, start)
    be = A.GpuBackend(seq)
    try:
        A.run(seq.calls, be, identity=True)
    finally:
        be.close()
    if kind != "dec":
        return
    # the cut census, read from last_cut() behind every call
    cut = {}
    for call, g in zip(seq.calls, be.cuts):
        if call.fam.cuts:
            cut.setdefault(call.op.family, [0, 0])[0 if g else 1] += 1
    behind = sorted({b.op.family for a, b, g in zip(seq.calls, seq.calls[1:], be.cuts) if a.fam.cuts and g})
    _note(f"cut census {ids(case)} (family cut/uncut): " + ", ".join(f"{f} {a}/{b}" for f, (a, b) in sorted(cut.items())) + "; behind a cut call: " + ", ".join(behind))
    if name == "2048x2x6":
        assert all(a >= 1 and b >= 1 for a, b in cut.values()), f"a streaming family never ran cut, or never uncut: {cut}"
        assert set(A.AFTER_CUT) <= set(behind), f"never directly behind a cut call: {sorted(set(A.AFTER_CUT) - set(behind))}"
    else:
        assert not any(a for a, _ in cut.values()), cut


def _filler(t, stream, seconds):
    """-> (a function that enqueues torch work of about `seconds` on the current stream and returns an event recorded behind it,
    the measured seconds of one unit, the units)"""
    x = t.randn(2048, 2048, device="cuda:0")
    y = t.empty_like(x)
    with t.cuda.stream(stream):
        t.mm(x, x, out=y)
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            t.mm(x, x, out=y)
        e1.record()
    stream.synchronize()
    unit = e0.elapsed_time(e1) / 20 / 1000.0
    units = max(1, math.ceil(seconds / unit))

    def enqueue():
        for _ in range(units):
            t.mm(x, x, out=y)
        ev = t.cuda.Event()
        ev.record()
        return ev
    return enqueue, unit, units


def _first_call_seconds(seq):
    """how long the chain's first call takes to return on a fresh object (its lazy pieces built inside it)"""
    import torch
    be = A.GpuBackend(seq)
    prepared = be.prepare(seq.calls[:1])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    be.enqueue(seq.calls[0], prepared[0], st)
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    be.close()
    return dt


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_sequence_on_one_stream_without_synchronisation(case):
    import torch
    kind, name, start = case
    seq = A.sequence(kind, name, start, device_only=True)
    calls = seq.calls
    assert not any(c.fam.host for c in calls)
    first = _first_call_seconds(seq)
    st = torch.cuda.Stream()
    filler, unit, units = _filler(torch, st, MARGIN * first)
    _note(f"filler {ids(case)}: the first call ({calls[0].op.family}) returns in {first * 1e3:.3f} ms on a fresh object; filler {units} x {unit * 1e3:.3f} ms "
          f"= {units * unit * 1e3:.3f} ms (margin {MARGIN})")
    be = A.GpuBackend(seq)
    try:
        for run in (1, 2):                                  # 1: the lazy pieces are built inside the chain; 2: everything is built
            prepared = be.prepare(calls)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                ev = filler()
                be.enqueue(calls[0], prepared[0], st)
                started = ev.query()
                for c, p in zip(calls[1:], prepared[1:]):
                    be.enqueue(c, p, st)
            st.synchronize()
            assert not started, f"run {run}: the device had passed the filler when the first call returned - the chain ran behind an idle stream"
            try:
                A.run(calls, A.Recorded(be.fetch(prepared)), identity=False)
            except A.AxisFailure as e:
                raise A.AxisFailure(f"run {run} of the chain: {e}") from None
            del prepared
            torch.cuda.synchronize()
            be.obj.reset()
            be.records.clear()
    finally:
        be.close()


def test_two_objects_interleaved():
    """The decoder and encoder sequences of the small geometry, call by call between those of a second pair of objects of the
    other geometry, on one stream: nothing is shared between objects - tables, __constant__ data, pick caches."""
    import torch
    N = 120
    seqs = [A.sequence("dec", "512x1x9", "a", device_only=True), A.sequence("enc", "512x1x9", "a", device_only=True),
            A.sequence("dec", "2048x2x6", "a", device_only=True), A.sequence("enc", "2048x2x70", "a", device_only=True)]
    bes = []
    try:
        for q in seqs:
            bes.append(A.GpuBackend(q, dec=bes[-1].obj if q.kind == "enc" else None))     # an encoder's clips calls take the decoder of its pair
        prepared = [be.prepare(q.calls[:N]) for be, q in zip(bes, seqs)]
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            for i in range(N):
                for be, q, p in zip(bes, seqs, prepared):
                    be.enqueue(q.calls[i], p[i], st)
        st.synchronize()
        for be, q, p in zip(bes, seqs, prepared):
            try:
                A.run(q.calls[:N], A.Recorded(be.fetch(p)), identity=False)
            except A.AxisFailure as e:
                raise A.AxisFailure(f"{q.kind} {q.name}, interleaved: {e}") from None
    finally:
        for be in bes:
            be.close()
