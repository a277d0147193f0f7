"""The file and corpus model every decoder-side family builds on (tests/corpus_testlib.py), held to the oracle directly and to
the layout rules of include/ulc_amd.h section 3, independent of any family: over every geometry of seek_testlib.geometries() and
over one corpus for each distinction the model makes by argument.  CPU only; the streams are the cached ones."""
import numpy as np
import pytest
from seek_testlib import SEED0, geometries, oracle_walk
from corpus_testlib import INDEX_DTYPE, PAD, Corpus, geom_files

GEOMS = sorted(geometries().keys())
STEREO = (2048, 2)
FOREIGN = 0xDEADBEEF


def _moved(f):
    """A copy of the file's payload with one byte changed, and of its offsets with one entry moved past the payload."""
    pay, offs = f.payload.copy(), f.offs.copy()
    pay[int(offs[3])] ^= 0x5A
    offs[5] = int(offs[-1]) + 40
    return pay, offs


def _corpora():
    a, b = geom_files(STEREO)
    pay, offs = _moved(a)
    return {"a None file": dict(files=[a, None, b]),
            "a None file in front": dict(files=[None, b]),
            "payload and offset overrides": dict(files=[a, b], payloads=[pay, b.payload], offs=[offs, b.offs]),
            "foreign states and slack": dict(files=[a, b], states=FOREIGN, index_slack=3),
            "equal-length files": dict(files=[a, a, a])}


CASES = [(f"{bs}x{ch}", dict(files=geom_files((bs, ch)))) for bs, ch in GEOMS] + list(_corpora().items())


def test_the_index_entry_is_the_librarys():
    from gpu_testlib import amd
    assert amd().INDEX_DTYPE == INDEX_DTYPE and INDEX_DTYPE.itemsize == 8


@pytest.mark.parametrize("geom", GEOMS)
def test_a_files_index_row_is_the_oracles_walk_of_its_payload(geom):
    bs, ch = geom
    for f in geom_files(geom):
        bits, offs, seeds, inside = oracle_walk(f.payload, f.payload.size, ch, bs, f.K + 2)
        assert inside and len(bits) == f.K, f.name
        assert np.array_equal(bits, f.obits) and np.array_equal((bits + 7) // 8, f.nb), f.name
        row = f.row()
        assert row.dtype == INDEX_DTYPE and row.shape == (f.K + 1,)
        assert np.array_equal(row["ByteOffs"], offs) and np.array_equal(row["RngState"], seeds), f.name
        assert row[0]["ByteOffs"] == 0 and row[0]["RngState"] == SEED0 and int(offs[-1]) == f.payload.size
        wide = f.row(cap=f.K + 4, blocks=f.K - 1)              # a row of more entries than blocks + 1, of fewer blocks than the file
        assert np.array_equal(wide[:f.K], row[:f.K]) and (wide["ByteOffs"][f.K:] == -1).all() and (wide["RngState"][f.K:] == 0).all()


@pytest.mark.parametrize("name,args", CASES, ids=[n for n, _ in CASES])
def test_both_layouts_hold_the_same_files(name, args):
    cor = Corpus(**args)
    files, F = args["files"], len(args["files"])
    states, slack = args.get("states"), args.get("index_slack", 0)
    K = [0 if f is None else f.K for f in files]
    pays = args.get("payloads") or [np.zeros(0, np.uint8) if f is None else f.payload for f in files]
    offs = args.get("offs") or [np.zeros(1, np.int64) if f is None else f.offs for f in files]
    assert cor.F == F and cor.K == K and np.array_equal(cor.count, K) and cor.count.dtype == np.int32
    assert np.array_equal(cor.nbytes, [len(p) for p in pays]) and cor.nbytes.dtype == np.int32
    # the strides
    longest = max(len(p) for p in pays)
    assert cor.stride % 16 == 0 and longest + PAD <= cor.stride < longest + PAD + 16
    assert cor.host.shape == (F, cor.stride) and cor.host.dtype == np.uint8
    assert cor.istride == max(K) + 1 + slack and cor.index.shape == (F, cor.istride) and cor.index.dtype == INDEX_DTYPE
    # the offset tables
    assert cor.poffs.dtype == cor.ioffs.dtype == np.int64 and cor.poffs[0] == cor.ioffs[0] == 0
    assert np.array_equal(np.diff(cor.poffs), [len(p) for p in pays]) and np.array_equal(np.diff(cor.ioffs), [k + 1 for k in K])
    assert cor.rpay.shape == (int(cor.poffs[-1]) + PAD,) and cor.rpay.dtype == np.uint8
    assert cor.ridx.shape == (int(cor.ioffs[-1]),) and cor.ridx.dtype == INDEX_DTYPE
    for i, f in enumerate(files):
        n, k = len(pays[i]), K[i]
        # one payload, twice, and zeros behind it
        assert np.array_equal(cor.host[i, :n], pays[i]) and not cor.host[i, n:].any(), (name, i)
        assert np.array_equal(cor.rpay[cor.poffs[i]:cor.poffs[i + 1]], pays[i]), (name, i)
        # one index row, twice: the offsets the buffers were given, the oracle's states (or the one foreign value), the fill
        row = cor.index[i]
        assert row[:k + 1].tobytes() == cor.ridx[cor.ioffs[i]:cor.ioffs[i + 1]].tobytes(), (name, i)
        assert np.array_equal(row["ByteOffs"][:k + 1], offs[i]), (name, i)
        want = np.full(k + 1, states, np.uint32) if states is not None else np.array([SEED0], np.uint32) if f is None else f.seeds
        assert np.array_equal(row["RngState"][:k + 1], want), (name, i)
        assert (row["ByteOffs"][k + 1:] == -1).all() and (row["RngState"][k + 1:] == (0 if states is None else states)).all(), (name, i)
        if f is None:
            assert n == 0 and row[0]["ByteOffs"] == 0 and row[0]["RngState"] == SEED0
    assert not cor.rpay[cor.poffs[-1]:].any()
    if name == "equal-length files":
        assert np.array_equal(cor.poffs, np.arange(F + 1) * len(pays[0])) and np.array_equal(cor.ioffs, np.arange(F + 1) * (K[0] + 1))
        assert cor.istride == K[0] + 1 and cor.ridx.tobytes() == cor.index.tobytes()
    lay, rag = cor.strided(), cor.ragged()
    assert lay["host"] is cor.host and lay["index"] is cor.index and rag["payload"] is cor.rpay and rag["index"] is cor.ridx
    assert np.array_equal(rag["blocks"], cor.count) and np.array_equal(lay["count"], cor.count)


def test_overrides_change_the_buffers_and_not_the_files():
    a, b = geom_files(STEREO)
    pay, offs = _moved(a)
    cor = Corpus([a, b], payloads=[pay, b.payload], offs=[offs, b.offs])
    clean = Corpus([a, b])
    assert not np.array_equal(cor.host[0], clean.host[0]) and np.array_equal(cor.host[1], clean.host[1])
    assert cor.index["ByteOffs"][0, 5] == offs[5] != a.offs[5] and np.array_equal(cor.index["RngState"], clean.index["RngState"])
    assert cor.stride == clean.stride and np.array_equal(a.payload, clean.host[0, :a.payload.size])


@pytest.mark.parametrize("geom", GEOMS)
def test_rows_outside_a_file_are_zeros(geom):
    fl = geom_files(geom)
    cor = Corpus(fl + [None])
    f, N = fl[0], 5
    none = len(fl)
    files = [0, 0, none, -1, cor.F, 0, 0]
    first = [f.K, 2, 0, 0, 0, f.K - 2, 2]
    count = [N, N, N, N, N, N, 2]
    pcm, pbits = cor.expected_pcm(files, first, N, count)
    coef, wc, sbits = cor.expected_spec(files, first, N, count)
    assert pcm.shape == (7, N, f.bs, f.ch) and coef.shape == (7, f.ch, N, f.bs) and wc.shape == pbits.shape == sbits.shape == (7, N)
    assert np.array_equal(pbits, sbits)
    for i in (0, 2, 3, 4):                                  # first = K, a None file, file numbers outside the corpus
        assert not pcm[i].any() and not coef[i].any() and not wc[i].any() and not pbits[i].any(), i
    assert (pbits[1] > 0).all() and (wc[1] != 0).all() and pcm[1].any() and coef[1].any()
    assert np.array_equal(pbits[1], f.obits[2:2 + N]) and np.array_equal(pcm[1], f.pcm[2:2 + N])
    assert np.array_equal(coef[1], f.coef[2:2 + N].transpose(1, 0, 2)) and np.array_equal(wc[1], f.wc[2:2 + N])
    assert (pbits[5, :2] > 0).all() and not pbits[5, 2:].any() and not pcm[5, 2:].any() and not coef[5][:, 2:].any() and not wc[5, 2:].any()   # the file's end
    assert (pbits[6, :2] > 0).all() and not pbits[6, 2:].any() and not pcm[6, 2:].any() and not coef[6][:, 2:].any() and not wc[6, 2:].any()   # behind count
    assert np.array_equal(pcm[6, :2], pcm[1, :2]) and np.array_equal(coef[6][:, :2], coef[1][:, :2])
    one = f.expected_pcm(f.K, N)
    assert not one[0].any() and not one[1].any()
