"""The census of the geometry axis, without a GPU: from the model (tests/geometry_axis_testlib.classes) and the oracle alone, every
case is in the class it is listed under, every class is reached by every call kind that can reach it, and the oracle's run of
every case holds the blocks the case is there for.  tests/test_gpu_geometry_axis.py runs the same list on the device.

`pytest -s` prints the census: per (selection class, kind) the cases that cover it and the blocks a GPU run compares."""
import itertools
import numpy as np
import pytest

import geometry_axis_testlib as G

CASE_IDS = [G.case_id(c) for c in G.CASES]


def _covered(kind, key):
    """{class value: [cases]} of the cases that run under a kind"""
    out = {}
    for bs, ch in G.cases_of(kind):
        out.setdefault(G.classes(bs, ch)[key], []).append((bs, ch))
    return out


def test_the_model_on_geometries_read_off_the_source():
    """Hand-read picks, one per branch of the rules (not the case list's own claims)."""
    want = {
        (2048, 2): dict(sel="W64c", xf="X2", wc="fused", gap="on", heap="lds"),                 # the benched shape
        (4096, 2): dict(sel="P128", xf="X2", wc="fused", gap="on", heap="lds"),
        (8192, 2): dict(sel="G", xf="X2", wc="fused", gap="on", heap="lds"),                    # R = 256; 16384 coefficients: the last with both
        (8192, 3): dict(sel="G", xf="Xn8192", wc="split", gap="off_by_size", heap="hbm"),
        (4096, 3): dict(sel="G", xf="Xn", wc="split", gap="on", heap="lds"),                    # R = 192
        (1024, 6): dict(sel="G", xf="Xn", wc="split", gap="on", heap="lds"),                    # R = 96
        (512, 4): dict(sel="W32", xf="Xn", wc="split", gap="on", heap="lds"),
        (256, 64): dict(sel="G", xf="Xn", wc="split", gap="off_by_channels", heap="lds"),       # 16384 coefficients, 64 channels
        (32768, 1): dict(sel="G", xf="XB", wc="split", gap="off_by_size", heap="hbm"),
        (16384, 2): dict(sel="G", xf="XB", wc="fused", gap="off_by_size", heap="hbm"),
    }
    for (bs, ch), w in want.items():
        assert G.classes(bs, ch) == w, f"{bs} x {ch}: {G.classes(bs, ch)}"


@pytest.mark.parametrize("case", G.CASES, ids=CASE_IDS)
def test_every_case_is_in_the_class_it_is_listed_under(case):
    bs, ch, sel = case
    c = G.classes(bs, ch)
    assert c["sel"] == sel, f"{bs} x {ch}: listed under {sel}, the model says {c}"
    assert all(c[k] in dom for k, dom in (("sel", G.SEL), ("xf", G.XF), ("wc", G.WC), ("gap", G.GAP), ("heap", G.HEAP)))
    # what the case list says of single cases
    notes = {(256, 16): dict(gap="on"), (256, 17): dict(gap="off_by_channels"), (256, 32): dict(gap="off_by_channels", heap="lds"),
             (2048, 9): dict(gap="off_by_size", heap="hbm", xf="Xn"), (8192, 3): dict(xf="Xn8192"), (16384, 1): dict(xf="XB")}
    for k, v in notes.get((bs, ch), {}).items():
        assert c[k] == v, f"{bs} x {ch}: {k} = {c[k]}, the case is there for {v}"


def test_the_first_geometry_beyond_each_limit_is_the_one_listed():
    assert G.classes(256, 16)["gap"] == "on" and G.classes(256, 17)["gap"] == "off_by_channels"
    assert G.classes(8192, 2)["gap"] == "on" and G.classes(2048, 9)["gap"] == "off_by_size"
    assert [ch for ch in range(1, 256) if G.classes(256, ch)["gap"] != "on"][0] == 17
    assert [ch for ch in range(1, 256) if G.classes(2048, ch)["heap"] != "lds"][0] == 9


def test_every_selection_class_under_every_call_kind(capsys):
    with capsys.disabled():
        print("\ngeometry census: (sel class, kind) -> cases, blocks a GPU run compares with the oracle")
        for sel in G.SEL:
            for kind in ("vbr", "search", "table", "ladder", "decode"):
                got = _covered(kind, "sel").get(sel, [])
                blocks = sum(G.blocks_compared(kind, ch) for _, ch in got)
                print(f"  {sel:5s} {kind:7s} {' '.join(G.case_id(c) for c in got):40s} {blocks}")
    for kind in ("vbr", "search", "table", "ladder", "decode"):
        assert set(_covered(kind, "sel")) == set(G.SEL), f"{kind}: classes without a case: {set(G.SEL) - set(_covered(kind, 'sel'))}"


def test_every_class_with_a_many_channel_geometry_has_one_in_a_table_call():
    """A class admits more than two channels when some (BlockSize, channels > 2) the header allows lies in it."""
    sizes = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
    admits = {G.classes(bs, ch)["sel"] for bs in sizes for ch in range(3, 256)}
    assert admits == set(G.SEL) - {"W4", "W8", "W64c", "P128"}         # 256 x 1, 256 x 2 / 512 x 1, stereo 2048 and stereo 4096 only
    have = {G.classes(bs, ch)["sel"] for bs, ch in G.cases_of("table") if ch > 2}
    assert have == admits, f"classes without a many-channel table case: {admits - have}"


def test_every_front_end_class_under_the_analysis_and_pcm16_kinds():
    for kind in ("analyse", "pcm16"):
        assert set(_covered(kind, "xf")) == set(G.XF), f"{kind}: transform classes without a case: {set(G.XF) - set(_covered(kind, 'xf'))}"
        assert set(_covered(kind, "wc")) == set(G.WC), f"{kind}: window-control classes without a case"


def test_every_gap_and_heap_pair_that_exists_under_the_exact_kind(capsys):
    sizes = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
    exists = {(G.classes(bs, ch)["gap"], G.classes(bs, ch)["heap"]) for bs in sizes for ch in range(1, 256)}
    assert exists == {("on", "lds"), ("off_by_channels", "lds"), ("off_by_size", "hbm")}     # (both limits are 16384 coefficients)
    have = {}
    for bs, ch in G.cases_of("exact"):
        c = G.classes(bs, ch)
        have.setdefault((c["gap"], c["heap"]), []).append((bs, ch))
    with capsys.disabled():
        print("\ngeometry census: exact path (gap, heap) -> cases")
        for k, v in have.items():
            print(f"  {k[0]:16s} {k[1]:4s} {' '.join(G.case_id(c) for c in v)}")
    assert set(have) == exists


@pytest.mark.parametrize("case", G.CASES, ids=CASE_IDS)
def test_the_oracles_run_of_a_case_holds_what_the_case_is_there_for(case):
    bs, ch, _ = case
    pcm = G.streams(bs, ch)
    assert pcm.shape == (G.B, G.NBLK * bs, ch)
    assert np.array_equal(pcm, np.clip(np.rint(pcm * 32768.0), -32768, 32767).astype(np.float32) * np.float32(2.0 ** -15)), "a stream off the PCM16 grid"
    silent = [s for s in range(G.B) if not pcm[s].any()]                # (mono: the 'last channel silent' stream is silent altogether)
    assert G.SILENT in silent and G.QUIET not in silent and len(silent) == (2 if ch == 1 else 1)
    assert 0 < np.abs(pcm[G.QUIET]).max() <= 2.0 ** -14
    refs = G.oracle_rows(bs, ch, G.VBR50)
    dec, undec = G.live_block_kinds(refs)
    kept = G.kept_per_stream(refs)
    print(f"{bs} x {ch}: {dec} decimated and {undec} un-decimated live blocks; blocks with nOutCoef > 0 per stream {kept}")
    assert dec >= 1 and undec >= 1, f"{dec} decimated, {undec} un-decimated live blocks: the masking levels take one path only"
    for s in range(G.B):
        if s in silent:
            assert kept[s] == 0, f"stream {s} is silent and keeps coefficients in {kept[s]} blocks"
            assert all(o["cplx"] == 0.0 for o in refs[s])
        else:
            assert 2 * kept[s] > G.NBLK, f"stream {s} keeps coefficients in {kept[s]} of {G.NBLK} blocks"
    # the rate searches really search: somewhere the CBR / ABR runs keep another count than VBR 50 keeps
    for setting in (G.cbr_of(ch), G.ABR96):
        other = G.oracle_rows(bs, ch, setting)
        assert any(o["nout"] != v["nout"] for r, rv in zip(other, refs) for o, v in zip(r, rv)), f"{setting} keeps what VBR 50 keeps"
    # the table: the CBR 32 row and the VBR 100 row keep different counts, and kSel is starved and saturated
    tab = G.oracle_rows(bs, ch, G.table_of(ch))
    cbr = [o["nout"] for o in tab[G.TABLE_CBR_ROW]]
    v100 = [o["nout"] for o in tab[G.TABLE_VBR100_ROW]]
    print(f"{bs} x {ch}: table rows keep CBR 32 {cbr}, VBR 100 {v100} of {ch * bs}")
    assert any(a != b for a, b in zip(cbr, v100)), "the CBR row and the VBR 100 row keep the same counts in every block"
    assert max(v100) == ch * bs, "VBR 100 never keeps every coefficient"
    assert max(cbr) < ch * bs // 8, "CBR 32 is no starved search"
    # the decode leg's reference exists (the oracle decodes its own streams)
    blocks, out, _ = G.oracle_decoded(bs, ch)
    assert blocks.shape == (G.B, G.NBLK, 2 * ch * bs + 16) and out.shape == pcm.shape


def test_comparer_names_stream_call_block_and_byte():
    bs, ch = 256, 3
    refs = G.oracle_rows(bs, ch, G.VBR50)
    K = G.CALLS[0]
    slot = 2 * ch * bs + 16
    out = np.zeros((G.B, K, slot), np.uint8)
    bits = np.array([[o["bits"] for o in r[:K]] for r in refs], np.int32)
    wc = np.array([[o["wc"] for o in r[:K]] for r in refs], np.int32)
    cplx = np.array([[o["cplx"] for o in r[:K]] for r in refs], np.float32)
    for s, k in itertools.product(range(G.B), range(K)):
        out[s, k, :bits[s, k] // 8] = refs[s][k]["bytes"]
    G.compare_call((out, bits, wc, cplx), refs, 0, 0, "model")
    bad = out.copy()
    bad[2, 1, 5] ^= 0x10
    with pytest.raises(AssertionError, match=r"stream 2 call 0 block 1 .*bytes differ from byte 5 of"):
        G.compare_call((bad, bits, wc, cplx), refs, 0, 0, "model")
    w2 = wc.copy(); w2[4, 2] ^= 1
    with pytest.raises(AssertionError, match=r"stream 4 call 0 block 2 .*WindowCtrl"):
        G.compare_call((out, bits, w2, cplx), refs, 0, 0, "model")
    c2 = cplx.copy(); c2[0, 1] = np.nextafter(c2[0, 1], np.float32(9))
    with pytest.raises(AssertionError, match=r"stream 0 call 0 block 1 .*BlockComplexity"):
        G.compare_call((out, bits, wc, c2), refs, 0, 0, "model")
    taps = dict(nout=np.array([[o["nout"] for o in r[:K]] for r in refs], np.int32), keep=np.stack([np.stack([o["keep"] for o in r[:K]]) for r in refs]))
    G.compare_call((out, bits, wc, cplx), refs, 0, 0, "model", taps, bs)
    taps["keep"] = taps["keep"].copy(); taps["keep"][3, 2, 2 * bs + 7] ^= 1
    with pytest.raises(AssertionError, match=r"stream 3 call 0 block 2 .*kept set differs from coefficient 519 \(channel 2\)"):
        G.compare_call((out, bits, wc, cplx), refs, 0, 0, "model", taps, bs)
