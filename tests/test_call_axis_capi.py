"""The call axis without a GPU (tests/call_axis_testlib.py): what the sequences hold, that the checker catches what it is for,
and that no entry point of the binding escapes the axis.  The GPU half is tests/test_gpu_call_axis.py."""
import os
import numpy as np
import pytest

import gpu_testlib                                          # (the path entry of ulc-codec_amd: the binding's tables, the cut's host arithmetic)
import call_axis_testlib as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EVIDENCE = os.path.join(ROOT, "profiles", "call_axis_evidence.txt")
CASES = [(kind, name, start) for kind in ("dec", "enc") for name in A.GEOMS[kind] for start in A.STARTS]
ids = lambda c: "-".join(c)


def _plain(v):
    return v[0] if isinstance(v, tuple) else v


# ---------------------------------------------------------------------------------------------------------------------
# 1. census
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_census_of_a_sequence(case):
    kind, name, start = case
    seq = A.sequence(kind, name, start)
    c = A.census(seq)
    F = len(c["names"])
    assert not c["missing_pairs"], f"ordered pairs of families that never occur as consecutive calls: {c['missing_pairs'][:5]}"
    assert len(seq.calls) == F * F + 1 + seq.prologue
    # K from {1, 3, maxK}, slot lists of 1, 5 and 65 (or all) slots, crop calls of at most 8 rows of at most 3 blocks
    Ks = {call.op.hint["K"] for call in seq.calls if "K" in call.op.p}
    assert Ks == {1, 3, seq.geom[3]}, Ks
    ns = {len(call.op.p["slots"]) for call in seq.calls if "subset" in call.op.family}
    assert {1, 5, min(65, seq.geom[2])} <= ns, ns
    for call in seq.calls:
        if "rows" in call.op.p and kind == "dec":
            assert len(call.op.p["rows"]) <= 8 and call.op.p.get("N", 3) <= 3
    # every slot has at least two lives, and the slots end at different positions
    assert min(c["lives"]) >= 2, c["lives"]
    assert len(set(c["positions"])) > 1, c["positions"]
    # every op's oracle reference is non-trivial: non-zero PCM / coefficients / payload bytes, live bits
    for call in seq.calls:
        for k, v in call.expected.items():
            v = _plain(v)
            if k in ("pcm", "bits", "coef", "out", "payload", "wc", "index", "dist", "out_payload", "out_index"):      # (not cplx: a stream's block 0 has complexity 0)
                assert np.count_nonzero(v) > 0, f"{call.op}: the expected {k} is all zero"
        if call.fam.streaming and "bits" in call.expected:
            assert (_plain(call.expected["bits"]) > 0).all(), f"{call.op}: a streaming call with a block of 0 bits"


@pytest.mark.parametrize("kind,name", [(k, n) for k in ("dec", "enc") for n in A.GEOMS[k]], ids=lambda v: v)
def test_every_lazy_piece_is_built_or_grown_in_both_positions(kind, name):
    """Start a builds and grows every lazy piece between two streaming calls, start b in front of the walk."""
    a, b = (A.census(A.sequence(kind, name, s))["lazy"] for s in A.STARTS)
    assert set(a) == set(b) and a, (sorted(a), sorted(b))
    want = {"dec": {"dec_shadow", "dec_low1", "dec_host_in", "dec_host_out", "resident_payload", "resident_index"},
            "enc": {"enc_shadow", "clips_staging", "clip_scratch", "clip_auto", "clip_spec", "enc_host_staging", "lad_staging"}}[kind]
    assert want <= set(a), want - set(a)
    for piece in a:
        assert [w for w, _, _ in a[piece]] == [w for w, _, _ in b[piece]], piece
        assert all(pos == "between" for _, _, pos in a[piece]), (piece, a[piece])
        assert all(pos == "front" for _, _, pos in b[piece]), (piece, b[piece])
    for piece in ("dec_host_in", "clips_staging", "lad_staging"):
        if piece in a:
            assert "grow" in [w for w, _, _ in a[piece]], f"{piece} never grows"


def test_streams_and_corpus_hold_what_the_kernels_branch_on():
    for name, (bs, ch, B, maxK) in A.DEC_GEOMS.items():
        wc = np.concatenate([A.dec_file(bs, ch, s).wc for s in range(B)])
        assert (wc & 8).any() and not (wc & 8).all(), f"{name}: the streams need decimated and un-decimated blocks"
        seq = A.sequence("dec", name, "a")
        cor = A.corpus(bs, ch)
        ends = dead = 0
        for call in seq.calls:
            for row in call.op.p.get("rows", ()):
                if call.op.family.startswith("decode_crops_lowrate"):
                    dead += row[0] == cor.F - 1
                elif call.op.family in ("decode_crops", "decode_crops_ragged", "decode_crops_spectra", "decode_crops_distortion"):
                    ends += row[1] + call.op.p["N"] > cor.K[row[0]]
        assert ends and dead, f"{name}: the corpus rows need an end of file ({ends}) and a dead block ({dead})"
    for name, (bs, ch, B, maxK) in A.ENC_GEOMS.items():
        wc = np.concatenate([A.enc_ref(bs, ch, s, A.VBR50)["wc"] for s in range(min(B, 9))])
        assert (wc & 8).any() and not (wc & 8).all(), name


def test_the_cut_census_of_the_long_row_decoder():
    """(2048, 2, 6, 24): by the library's own plan arithmetic every streaming family runs cut and uncut, and each of save, load,
    reset, subset, packed, range and a stateless family runs directly behind a cut call.  (512, 1): never cut."""
    for start in A.STARTS:
        c = A.census(A.sequence("dec", "2048x2x6", start))
        fams = A.families("dec", A.DEC_GEOMS["2048x2x6"])
        assert set(c["cut"]) == {n for n in fams if fams[n].cuts}
        assert all(cut >= 1 and uncut >= 1 for cut, uncut in c["cut"].values()), c["cut"]
        assert set(A.AFTER_CUT) <= set(c["behind_cut"]), set(A.AFTER_CUT) - set(c["behind_cut"])
        assert not any(cut for cut, _ in A.census(A.sequence("dec", "512x1x9", start))["cut"].values())


MEASURED = "== measured on an MI355X =="


def _census_text():
    lines = ["== the sequences =="]
    for kind, name, start in CASES:
        seq = A.sequence(kind, name, start)
        c = A.census(seq)
        lines += A.pair_matrix(seq)
        lines += ["  lazy pieces (piece: what, at call, position): " + "; ".join(f"{p}: " + ", ".join(f"{w} at {i} {pos}" for w, i, pos in ev) for p, ev in sorted(c["lazy"].items()))]
        if kind == "dec":
            lines += ["  planned cut census (family: cut calls / uncut calls): " + ", ".join(f"{f} {a}/{b}" for f, (a, b) in sorted(c["cut"].items())),
                      "  directly behind a cut call: " + ", ".join(c["behind_cut"])]
        lines += [f"  lives per slot {min(c['lives'])} .. {max(c['lives'])}; end positions {sorted(set(c['positions']))}", ""]
    return "\n".join(lines).rstrip()


def test_evidence_file_holds_the_census():
    """profiles/call_axis_evidence.txt: the pair matrix, the lazy-piece table and the planned cut census of every sequence - the
    committed file says what this tree's sequences are (its last section, the GPU's figures, is written on an MI355X)."""
    have = open(EVIDENCE).read() if os.path.exists(EVIDENCE) else ""
    assert have.split(MEASURED)[0].rstrip() == _census_text(), \
        "profiles/call_axis_evidence.txt is not this tree's census (python tests/test_call_axis_capi.py writes it)"


# ---------------------------------------------------------------------------------------------------------------------
# 2. the checker catches what it is for
# ---------------------------------------------------------------------------------------------------------------------
def test_a_stand_in_made_of_the_model_passes():
    for kind, name in (("dec", "512x1x9"), ("enc", "512x1x9")):
        seq = A.sequence(kind, name, "a")
        A.run(seq.calls, A.StandIn(seq))


@pytest.mark.parametrize("start", A.STARTS)
@pytest.mark.parametrize("fault,kind,name,family", [("stale_set", "dec", "2048x2x6", None), ("shadow_back", "dec", "512x1x9", None),
                                                    ("lost_chunk", "enc", "512x1x9", "ladder")])
def test_a_planted_fault_is_reported_with_its_place(fault, kind, name, family, start):
    """StandIn's three faults: (a) after a cut call save_streams reads the old state set, (b) a stateless family writes one slot's
    shadow state back, (c) growing the rung staging loses what was staged.  The message names the call, the pair of families and
    whether the call was the first of its family on the object."""
    seq = A.sequence(kind, name, start)
    with pytest.raises(A.AxisFailure) as e:
        A.run(seq.calls, A.StandIn(seq, fault))
    msg = str(e.value)
    i = int(msg.split(",")[0].split()[1])
    call = seq.calls[i]
    assert msg.startswith(f"op {i}, {call.op.prev} -> {call.op.family} ("), msg
    assert ("the first" if call.op.first else "not the first") + f" {call.op.family} call of the object" in msg, msg
    if family:
        assert family in call.op.family, msg
    if fault == "shadow_back":
        assert not call.fam.streaming or "subset" not in call.op.family, msg


# ---------------------------------------------------------------------------------------------------------------------
# 3. ops against the binding
# ---------------------------------------------------------------------------------------------------------------------
def test_every_dev_entry_that_takes_an_object_is_sequenced_or_listed_with_a_reason():
    """A new entry point cannot be added to the binding without the axis noticing."""
    import ctypes as C
    amd = gpu_testlib.amd()
    sequenced = {e for fams in A.FAMILIES.values() for f in fams.values() for e in f.exports}
    entries = {n: sig for table in (amd.SIGNATURES, amd.EXT_SIGNATURES) for n, sig in table.items()}
    assert sequenced <= set(entries), f"families name entries the binding does not have: {sorted(sequenced - set(entries))}"
    assert set(A.NOT_SEQUENCED) <= set(entries), sorted(set(A.NOT_SEQUENCED) - set(entries))
    assert not sequenced & set(A.NOT_SEQUENCED), sorted(sequenced & set(A.NOT_SEQUENCED))
    dev = [n for n, (argtypes, _) in entries.items() if "_dev" in n and argtypes and argtypes[0] is C.c_void_p]
    assert len(dev) > 50, len(dev)
    stray = [n for n in dev if n not in sequenced and n not in A.NOT_SEQUENCED]
    assert not stray, f"_dev entries that take an object and are neither in a family of the call axis nor in NOT_SEQUENCED: {stray}"
    assert all(isinstance(r, str) and len(r) > 10 for r in A.NOT_SEQUENCED.values())
    assert len(A.NOT_SEQUENCED) <= 20
    assert {"ulcx_encode_block1", "ulcx_decode_block1", "ulcx_decode_block1_rng", "ulcx_encoder_debug_fetch"} <= set(A.NOT_SEQUENCED)


if __name__ == "__main__":                                  # writes the census part of the evidence file, keeps the measured part
    have = open(EVIDENCE).read() if os.path.exists(EVIDENCE) else ""
    tail = MEASURED + have.split(MEASURED)[1] if MEASURED in have else ""
    open(EVIDENCE, "w").write(_census_text() + "\n\n" + tail)
