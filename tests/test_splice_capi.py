"""Corpus splice (include/ulc_amd.h section 2: ulcx_corpus_splice_*) at the C-ABI boundary, without a GPU: the four entries'
presence, the refusals that need no device, and the premises of tests/test_gpu_splice.py's inputs - asserted here on the oracle
alone."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import splice_testlib as S
from seek_testlib import oracle_pcm, oracle_seeds

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_corpus_splice_dev", "ulcx_corpus_splice_ragged_dev", "ulcx_corpus_splice_host", "ulcx_corpus_splice_ragged_host")
ERR_ARG, ERR_NO_DEVICE = -1, -2
P, I, LL = C.c_void_p, C.c_int, C.c_longlong


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    return l


def test_splice_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    import corpus
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("corpus_splice", "corpus_splice_ragged", "corpus_splice_dev", "corpus_splice_ragged_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    assert ulc_amd.SEGMENT_DTYPE.itemsize == 12 and ulc_amd.SEGMENT_DTYPE == S.SEGMENT_DTYPE
    for m in ("splice", "trim", "switch"):
        assert hasattr(corpus.CropCorpus, m), m


def test_header_compiles_as_c_and_declares_the_calls():
    out = 'int, const int32_t *, const ulcx_segment *, int, uint8_t *, long long, int32_t *, int32_t *, ulcx_index_entry *, int, int32_t *, int32_t *'
    strided = 'ulcx_decoder *, int, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *, '
    ragged = 'ulcx_decoder *, int, const uint8_t *, long long, const int64_t *, const ulcx_index_entry *, long long, const int64_t *, const int32_t *, '
    src = ('#include "ulc_amd.h"\n'
           f'int (*a)({strided}{out}, void *) = ulcx_corpus_splice_dev;\n'
           f'int (*b)({strided}{out}) = ulcx_corpus_splice_host;\n'
           f'int (*c)({ragged}{out}, void *) = ulcx_corpus_splice_ragged_dev;\n'
           f'int (*d)({ragged}{out}) = ulcx_corpus_splice_ragged_host;\n'
           '_Static_assert(sizeof(ulcx_segment) == 12, "three int32");\n'
           'ulcx_segment s = { .File = 1, .First = 2, .Count = 3 };\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


# ---------------------------------------------------------------------------------------------------------------------
# refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_without_a_device_no_object_exists_and_the_entries_refuse(lib):
    """Without a device ulcx_decoder_create returns ULCX_ERR_NO_DEVICE and leaves no object, so every splice entry is refused
    before anything touches a device; which argument the refusal names shows the order of the checks - NULL pointers, the counts,
    the source's scalars, the output's, alignment, the overlap, and only then the missing decoder (ULCX_ERR_ARG, as
    tests/test_index_slots_capi.py finds for its calls)."""
    if lib.ulcx_device_count() <= 0:
        h = C.c_void_p()
        lib.ulcx_decoder_create.argtypes = [C.POINTER(C.c_void_p), I, I, I, I, I]
        assert lib.ulcx_decoder_create(C.byref(h), 0, 1, 2, 2048, 4) == ERR_NO_DEVICE and not h.value
    buf = (C.c_uint8 * 4096)()
    base = (C.addressof(buf) + 15) & ~15
    pay, idx, n4, t8 = base, base + 256, base + 512, base + 768
    opay, oidx, on4, om4, oc4, ss = base + 1024, base + 2048, base + 3072, base + 3136, base + 3200, base + 3264
    tail = [I, P, P, I, P, LL, P, P, P, I, P, P]
    forms = []
    for name, head, last in (("ulcx_corpus_splice_dev", [P, I, P, LL, P, P, I, P], [P]), ("ulcx_corpus_splice_host", [P, I, P, LL, P, P, I, P], []),
                             ("ulcx_corpus_splice_ragged_dev", [P, I, P, LL, P, P, LL, P, P], [P]),
                             ("ulcx_corpus_splice_ragged_host", [P, I, P, LL, P, P, LL, P, P], [])):
        fn = getattr(lib, name)
        fn.argtypes = head + tail + last
        forms.append((name, fn, "ragged" in name, "host" in name, [None] * len(last)))

    def call(fn, ragged, last, nFiles=2, pay=pay, nb=n4, idx=idx, cnt=n4, stride=64, istride=5, poffs=t8, ioffs=t8, ptotal=64, itotal=8,
             nOut=1, so=n4, seg=n4, nSeg=1, opay=opay, ostride=64, ob=on4, om=om4, oidx=oidx, oistride=4, oc=oc4, ss=ss):
        out = (nOut, so, seg, nSeg, opay, ostride, ob, om, oidx, oistride, oc, ss)
        if ragged:
            return fn(None, nFiles, pay, ptotal, poffs, idx, itotal, ioffs, cnt, *out, *last)
        return fn(None, nFiles, pay, stride, nb, idx, istride, cnt, *out, *last)

    for name, fn, ragged, host, last in forms:
        def refused(why, **kw):
            assert call(fn, ragged, last, **kw) == ERR_ARG, (name, kw)
            msg = lib.ulcx_last_error().decode()
            assert msg.startswith(name + ":") and why in msg, (name, kw, msg)
        for k in ("pay", "idx", "cnt", "so", "seg", "opay", "ob", "oidx", "oc", "ss") + (("poffs", "ioffs") if ragged else ("nb",)):
            refused("NULL pointer", **{k: None}, nFiles=0, nOut=0, nSeg=0)
        refused("nFiles 0", nFiles=0, stride=0, ostride=0)
        refused("nOut -1", nOut=-1)
        refused("nSeg 0", nSeg=0, oistride=1)
        if ragged:
            refused("payloadTotal -1", ptotal=-1, ostride=0)
            refused("indexTotal -5", itotal=-5)
        else:
            refused("payloadStride 0", stride=0, ostride=0)
            refused("indexStride 0", istride=0)
        refused("outPayloadStride 0", ostride=0)
        refused("outIndexStride 1", oistride=1)
        if not host:
            words = dict(cnt=n4, so=n4, seg=n4, ob=on4, om=om4, oidx=oidx, oc=oc4, ss=ss, idx=idx, **({} if ragged else {"nb": n4}))
            for k, at in words.items():
                refused("not aligned", **{k: at + 2})
            if ragged:
                refused("not aligned", poffs=t8 + 4)
                refused("not aligned", ioffs=t8 + 4)
            refused("overlaps", opay=pay + 8)               # the output payload inside the source's
            refused("overlaps", oidx=pay)                   # the output index over the source payload
            refused("overlaps", opay=idx - 32)              # the output payload running into the source index
            refused("overlaps", oidx=idx + 8)
            assert call(fn, ragged, last, om=None) == ERR_ARG and "no decoder" in lib.ulcx_last_error().decode()     # (d_outMaxBlock is optional)
        refused("no decoder")


# ---------------------------------------------------------------------------------------------------------------------
# the premises of the GPU tests' inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_a_trimmed_head_changes_the_noise_of_every_block_behind_it():
    """Blocks 5 .. of the stereo 2048 stream decoded as a file of their own differ from the same blocks inside the source's
    sequential decode, in every one of the first six blocks: the generator's state in front of a block depends on the blocks in
    front of it, so a splice has to rebuild the chain (test 2 of tests/test_gpu_splice.py)."""
    src = S.source(S.STEREO)
    f = src.files[0]
    whole, _ = oracle_pcm(f.blocks, 2, 2048)
    own, _ = oracle_pcm(f.blocks[5:], 2, 2048)
    differ = [k for k in range(6) if not np.array_equal(own[k], whole[5 + k])]
    assert differ == list(range(6)), differ
    seeds_whole, seeds_own = oracle_seeds(f.blocks, 2, 2048), oracle_seeds(f.blocks[5:], 2, 2048)
    assert all(seeds_own[k] != seeds_whole[5 + k] for k in range(6))
    e = S.expected(src, [[(0, 5, f.K - 5)]], 1 << 20, f.K + 1)[0][0]
    assert e.pcm.tobytes() == own.tobytes()


def test_the_two_rungs_of_a_clip_carry_the_same_window_codes():
    """synth_pcm(3, 40 * 2048, 2, 44100, transient=True, seed=11) at VBR 50 and VBR 20: equal window codes with at least three
    switched blocks - what makes a block-wise switch between rungs a stream whose aliasing cancels at every joint."""
    src, wc = S.switch_source()
    assert np.array_equal(wc[0], wc[1]) and int((wc[0] != 0x10).sum()) >= 3
    assert int((wc[0] != 0x10).sum()) == 4
    assert src.files[0].K == src.files[1].K == 40 and not np.array_equal(src.files[0].nb, src.files[1].nb)
    assert S.alternate(40, 1)[:3] == [(0, 0, 1), (1, 1, 1), (0, 2, 1)] and S.alternate(40, 4)[-1] == (1, 36, 4) and len(S.alternate(40, 4)) == 10


def test_every_alignment_pair_of_the_copy_occurs_in_one_output_file():
    blocks = S.alignment_blocks()
    pairs, nbytes = S.alignment_pairs(blocks)
    assert len(pairs) == 256, len(pairs)
    assert len(blocks) <= 600 and nbytes <= 160 * 1024, (len(blocks), nbytes)
    # the oracle-encoded stream alone does not reach them all: both files are needed
    src = S.source(S.STEREO)
    alone = {(int(src.files[0].offs[k]) % 16, d) for k in range(src.files[0].K) for d in range(16)}
    assert len(alone) < 256


def test_the_sources_and_the_rule():
    for geom in S.GEOMS:
        src = S.source(geom)
        assert src.F == 2 and {f.K for f in src.files} <= {40, 24}
        assert all(S.takes(src, f, k) for f in range(2) for k in (0, src.files[f].K - 1))
        names = [n for n, _ in S.shapes(src)]
        assert len(set(names)) == len(names) == 12
        segs = dict(S.shapes(src))
        assert len(segs["130 one-block segments"]) == 130 and sum(c for _, _, c in segs["file 0 three times"]) > 64
    src = S.source(S.STEREO)
    K = src.files[0].K
    # the rule: a count running past the end keeps its leading blocks, and nothing behind it is taken
    assert S.taken(src, [(0, K - 2, 5), (1, 0, 3)], 1 << 20, 100) == [(0, K - 2), (0, K - 1)]
    assert S.taken(src, [(0, 0, 2), (1, 0, -4), (0, 2, 0), (1, 3, 1)], 1 << 20, 100) == [(0, 0), (0, 1), (1, 3)]
    assert S.taken(src, [(0, 0, 2), (2, 0, 1), (1, 3, 1)], 1 << 20, 100) == [(0, 0), (0, 1)]
    assert S.taken(src, [(0, 0, 6)], 1 << 20, 5) == [(0, k) for k in range(4)]
    two = int(src.files[0].offs[2])
    assert S.taken(src, [(0, 0, 6)], two, 100) == [(0, 0), (0, 1)] and S.taken(src, [(0, 0, 6)], two - 1, 100) == [(0, 0)]
    assert S.plan_starts([(0, 0, 2), (1, 0, -4), (0, 2, 0), (1, 3, 1)]) == [0, 2, 2, 2]
    assert S.plan_starts([(0, 0, 2 ** 31 - 1), (0, 0, 5), (0, 0, 1)]) == [0, 2 ** 31 - 1, 2 ** 31 - 1]
    pats, which = S.many_patterns()
    assert len(which) == 16389 and set(which.tolist()) == set(range(24)) and {c for _, _, c in pats} == {1, 2, 3}
