"""Oracle references of the clips ladder tests (tests/test_clips_ladder_capi.py, tests/test_gpu_clips_ladder.py,
tests/test_gpu_clips_ladder_paths.py): what ulcx_encode_clips_ladder_* must write for clip i under rung r, from the oracle alone -
clips_testlib.ClipRef of the clip under the rung's setting for that row.  A ULCX_RUNG_AUTO rung's setting is
{RateKbps, avg_i}, avg_i = (float)(S_i / nb_i) formed here exactly as the header states it: S_i the binary64 sum of the oracle's
BlockComplexity values of the clip's nb_i blocks, added one after the other in block order.  The references are CPU only; LadderCall and its checks (at the end) are the
GPU tests' call on a guarded arena."""
import functools
import numpy as np
import clips_testlib as ct
import clip_spectra_testlib as cst
import guarded_buffers as gb
from ulc_testlib import to_pcm16
from gpu_testlib import amd as _amd, dev as _dev

# A rung of the tests: ("scalar", (RateKbps, AvgComplexity)) in the tool's convention, ("table",) = clips_testlib.TABLE,
# ("auto", kbps) = AUTO on a scalar rung, ("auto_table",) = AUTO on TABLE.
VBR50, TABLE, CBR64, AUTO96, AUTO_TABLE, AUTO64 = ("scalar", (-50.0, 0.0)), ("table",), ("scalar", (64.0, 0.0)), ("auto", 96.0), ("auto_table",), ("auto", 64.0)
FIVE = (VBR50, TABLE, CBR64, AUTO96, AUTO_TABLE)
# eight rungs: the five, then three of them again in another order (a rung must not depend on its place; the oracle runs are shared)
EIGHT = FIVE + (AUTO96, VBR50, CBR64)
PATH_RUNGS = (VBR50, AUTO64, TABLE)                         # tests/test_gpu_clips_ladder_paths.py, part A; TABLE is the highest-rate rung
GRID_RUNGS = (VBR50, TABLE)


def is_auto(rung):
    return rung[0] in ("auto", "auto_table")


def avg_of(cplx):
    """(float)(sum / nb): a sequential binary64 sum in block order, divided in binary64, rounded to binary32; 0 for no blocks."""
    s = 0.0
    for x in cplx:
        s += float(x)
    return np.float32(s / len(cplx)) if len(cplx) else np.float32(0.0)


@functools.lru_cache(maxsize=None)
def avg(bs, ch, i, case=None):
    """avg_i of pair i, from the oracle's complexities of the whole clip."""
    return avg_of(cst.row_spec(bs, ch, i, case).cplx)


def setting(bs, ch, i, rung, case=None, avg_row=None):
    """{RateKbps, AvgComplexity} of pair i under the rung.  avg_row: the pair whose average an AUTO rung uses (default: its own)."""
    a = float(avg(bs, ch, i if avg_row is None else avg_row, case)) if is_auto(rung) else 0.0
    if rung[0] == "scalar":
        return rung[1]
    if rung[0] == "table":
        return ct.TABLE[i]
    if rung[0] == "auto":
        return (rung[1], a)
    r = ct.TABLE[i]
    return r if r[0] < 0 else (r[0], a)


@functools.lru_cache(maxsize=None)
def _ref(bs, ch, i, case, st):
    case = case or ct.short_case(bs)
    return ct.ClipRef(bs, ch, ct.wave(bs, ch, case.T)[i][:, :case.lengths[i]], st)


def file_ref(bs, ch, i, rung, case=None):
    """Pair i under the rung (shared by the tests; nobody writes to it).  The scalar VBR 50 and TABLE references are
    clips_testlib's own, so the clips tests' oracle runs are not repeated."""
    if rung == VBR50 or rung == TABLE:
        return ct.row_ref(bs, ch, i, rung == TABLE, case)
    return _ref(bs, ch, i, case, tuple(float(x) for x in setting(bs, ch, i, rung, case)))


def refs(bs, ch, rungs, case=None, rows=None):
    """[R][n] references of a call: file r * n + j is refs[r][j]."""
    rows = range(7) if rows is None else rows
    return [[file_ref(bs, ch, i % 7, g, case) for i in rows] for g in rungs]


def lib_rungs(rungs, table_ptr=None, auto=True):
    """The rungs as BatchEncoder.encode_clips_ladder(_dev) takes them.  table_ptr: what stands for TABLE (a device address, or
    the host table of the call's rows)."""
    out = []
    for g in rungs:
        if g[0] == "scalar":
            out.append((0, -g[1][0]) if g[1][0] < 0 else (1, g[1][0]) if g[1][1] == 0 else (2, g[1][0], g[1][1]))
        elif g[0] == "table":
            out.append(table_ptr)
        elif g[0] == "auto":
            out.append(("auto", g[1]))
        else:
            out.append(("auto_table", table_ptr))
    return out


def ladder_cut(bs, ch):
    """The payload capacity of the GPU capacity test: (hi, lo, m, payloadStride) - one byte short of block m (in a chunk of 2
    behind the first) of row 6 under its highest-rate rung hi, while row 6 under its lowest-rate rung lo still fits whole."""
    rf = refs(bs, ch, FIVE)
    size = [rf[r][6].payload.size for r in range(5)]
    hi, lo = int(np.argmax(size)), int(np.argmin(size))
    for m in range(2, 8):
        stride = int(rf[hi][6].sizes[:m + 1].sum()) - 1
        if stride >= size[lo]:
            return hi, lo, m, stride
    raise AssertionError(f"no block of the highest-rate rung ends behind the lowest-rate rung's file: {size}")


# ---------------------------------------------------------------------------------------------------------------------
# The call on a guarded arena and its checks, for the GPU tests (torch and the library are imported when a call is made)
# ---------------------------------------------------------------------------------------------------------------------
N, B = 7, 8                                                 # rows of a call and streams of the object, unless a test says otherwise


class LadderCall:
    """One ulcx_encode_clips_ladder_dev(_pcm16) call on a guarded arena -> the outputs as numpy, [R * n]...  rungs: of
    clips_ladder_testlib; n rows on an object of `streams` streams; case / rows as tests/test_gpu_clips.py's Call takes them."""

    def __init__(self, enc, dec, bs, ch, rungs, pstride=None, istride=None, pcm16=False, null_len=False, null_opt=False, n=N, streams=B, case=None, rows=None):
        case = case or ct.short_case(bs)
        rows = [i % 7 for i in range(n)] if rows is None else list(rows)
        assert len(rows) == n <= streams
        T, nb = case.T, ct.clip_blocks(bs, case.T)
        R = len(rungs)
        F = self.F = R * n
        G = min(streams, 8)                                 # rows of a guard (the guards of a large object: as those of eight streams)
        self.n, self.R, self.T, self.rows, self.case, self.rungs = n, R, T, rows, case, rungs
        self.pstride = pstride or enc.slot * nb
        self.istride = istride or nb + 1
        self.auto = any(is_auto(g) for g in rungs)
        esz = 2 if pcm16 else 4
        word = lambda name, k, role: dict(name=name, nbytes=4 * k, align=4, role=role, guard=4 * G, row=4)
        specs = [dict(name="d_pcm", nbytes=n * ch * T * esz, align=esz, role="in", guard=G * ch * T * esz, row=T * esz, rows_per_stream=ch)]
        if not null_len:
            specs.append(word("d_len", n, "in"))
        if any(g[0] in ("table", "auto_table") for g in rungs):
            specs.append(dict(name="d_rate", nbytes=8 * n, align=8, role="in", guard=8 * G, row=8))
        specs += [dict(name="d_payload", nbytes=F * self.pstride, align=1, role="out", guard=G * self.pstride, row=self.pstride),
                  word("d_payloadBytes", F, "out"),
                  dict(name="d_index", nbytes=8 * F * self.istride, align=4, role="out", guard=8 * G * self.istride, row=8, rows_per_stream=self.istride),
                  word("d_indexBlocks", F, "out")]
        if not null_opt:
            specs += [word("d_maxBlock", F, "out"), word("d_avg", n, "out")]
        a = self.a = gb.build(_dev(), specs)
        w = ct.wave(bs, ch, T)[rows]
        a.load("d_pcm", to_pcm16(w) if pcm16 else w)
        if not null_len:
            a.load("d_len", np.array(case.lengths, np.int32)[rows])
        if "d_rate" in a.regions:
            a.load("d_rate", np.array(ct.TABLE, np.float32)[rows])          # (the caller's table: const, AUTO must not write it - check() holds it)
        self.lib_rungs = lib_rungs(rungs, a.ptr("d_rate") if "d_rate" in a.regions else None)
        self.pcm16, self.enc, self.dec = pcm16, enc, dec

    def run(self):
        import torch
        a = self.a
        opt = lambda name: a.ptr(name) if name in a.regions else 0
        self.enc.encode_clips_ladder_dev(self.dec, self.n, self.lib_rungs, a.ptr("d_pcm"), opt("d_len"), self.T, a.ptr("d_payload"), self.pstride,
                                         a.ptr("d_payloadBytes"), a.ptr("d_index"), self.istride, a.ptr("d_indexBlocks"), d_max_block=opt("d_maxBlock"),
                                         d_avg=opt("d_avg"), pcm16=self.pcm16)
        torch.cuda.synchronize()
        a.check()
        self.payload = a.fetch("d_payload").reshape(self.F, self.pstride)
        self.poison = gb.pattern(a.regions["d_payload"].off, self.F * self.pstride).reshape(self.F, self.pstride)
        self.nbytes, self.count = a.fetch("d_payloadBytes", np.int32), a.fetch("d_indexBlocks", np.int32)
        self.maxb = a.fetch("d_maxBlock", np.int32) if "d_maxBlock" in a.regions else None
        self.index = a.fetch("d_index", ct.INDEX_DTYPE).reshape(self.F, self.istride)
        if "d_avg" in a.regions:
            self.avg = a.fetch("d_avg", np.float32)
            self.avg_poison = gb.pattern(a.regions["d_avg"].off, 4 * self.n).view(np.float32)
        return self


def check_files(got, refs, what):
    """Every file against the oracle: the leading blocks the call's capacities keep, nothing written behind them.  refs [R][n]."""
    n = got.n
    for r in range(got.R):
        for i in range(n):
            f, ref = r * n + i, refs[r][i]
            m = ref.kept(got.pstride, got.istride)
            nbytes = int(ref.sizes[:m].sum())
            where = f"{what}: file {f} = rung {r}, row {i} ({ref.L} samples, {ref.nb} blocks, {m} kept)"
            assert got.count[f] == m, f"{where}: d_indexBlocks {got.count[f]}"
            assert got.nbytes[f] == nbytes, f"{where}: d_payloadBytes {got.nbytes[f]} vs the oracle's {nbytes}"
            if got.maxb is not None:
                assert got.maxb[f] == (int(ref.sizes[:m].max()) if m else 0), f"{where}: d_maxBlock {got.maxb[f]}"
            if not np.array_equal(got.payload[f, :nbytes], ref.payload[:nbytes]):
                bad = np.flatnonzero(got.payload[f, :nbytes] != ref.payload[:nbytes])
                edges = np.concatenate([[0], np.cumsum(ref.sizes)])
                raise AssertionError(f"{where}: {bad.size} of {nbytes} payload bytes differ from the oracle's, first at byte {bad[0]} "
                                     f"(block {int(np.searchsorted(edges, bad[0], 'right')) - 1}), last at {bad[-1]}")
            assert np.array_equal(got.payload[f, nbytes:], got.poison[f, nbytes:]), f"{where}: bytes behind the file's end were written"
            want = ref.index_row(got.istride, m)
            assert got.index[f].tobytes() == want.tobytes(), f"{where}: index {got.index[f][:m + 2]} vs the oracle's walk {want[:m + 2]}"


def check_avg(got, bs, ch, what):
    """d_avg bit for bit: the averages formed in Python from the oracle's complexities; untouched poison without an AUTO rung."""
    if got.auto:
        want = np.array([avg(bs, ch, i, got.case) for i in got.rows], np.float32)
        assert got.avg.tobytes() == want.tobytes(), f"{what}: d_avg {got.avg} vs {want}"
    else:
        assert got.avg.tobytes() == got.avg_poison.tobytes(), f"{what}: d_avg written without an AUTO rung"
