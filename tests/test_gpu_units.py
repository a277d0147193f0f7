"""The small pure device functions the bit-exactness claim rests on, run ON THE DEVICE one by one through the test-only
module libulcx_units.so (ulc-codec_amd/csrc/ulcx_units.hip: thin kernels around the product's own definitions, compiled
with the product's flags) and compared bit for bit with a plain reference of the same operation - over input domains far
wider than any audio signal reaches.  A failure names the function and the first failing input.

References:  the live glibc for the libm restatement (after the host compile of the same header has agreed with it on the
same grids - else this machine's glibc is not the 2.35 FMA variant and cannot referee); the oracle's helpers, pinned to
the reference by tests/test_oracle_pinned.py, for the scalar helpers and the noise-fill parameters; numpy branch cascades
and loops written from the format's code table for the syntax functions; GF(2) matrix powers and the oracle's generator
for rng_jump; numpy prefix operations for the wave primitives.

Domains.  Where C leaves the reference undefined the comparison is left out, the sweep's count of such patterns is
computed here and must equal what the referee skipped (tests/helpers/units_ref.c):
  quant_u / quant_coef_u / quant_coef   (int) of 0.5f + sqrtf(|v| - 0.25f) needs that value < 2^31, i.e. |v| < 2^62
                                        (C leaves the conversion undefined there: x86 gives INT_MIN, the device's
                                        conversion saturates at INT_MAX.  Outside what the codec reaches - the arguments are
                                        amplitudes times a quantiser scale - so documented, not patched); NaN is inside the
                                        domain (result 0)
  build_quantizer                       0 < maxv < inf (at +-0 the device gives 31 where x86 gives 5: logf is -inf, the conversion
                                        of +inf saturates; the writer calls it with the largest magnitude of kept coefficients)
  to_pcm16                              finite arguments
fastlog, key_ord, decode_code, plain_prefix, rng_jump and the wave primitives are total."""
import ctypes as C

import numpy as np
import pytest

import units_testlib as U
from units_testlib import (UF_EXPF, UF_EXPF_T, UF_LOGF, UF_FASTLOG, UF_QUANT_U, UF_QUANT_COEF_U, UF_QUANT_COEF, UF_BUILD_QUANTIZER,
                           UF_TO_PCM16, UF_KEY_ORD, UF_EXPAND_QUANTIZER, CODE_FIELDS, ptr)

pytestmark = pytest.mark.gpu

SWEEP = (0, 1 << 32, 61)              # every 61st pattern of the binary32 space: 70 M points, NaN / inf / subnormals included


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def bits_of(x):
    return np.asarray(x, np.float32).view(np.uint32)


def around(centres, ulps):
    """the patterns within `ulps` of each centre (float32 values), both signs untouched"""
    c = bits_of(np.asarray(centres, np.float32)).astype(np.int64)
    p = (c[:, None] + np.arange(-ulps, ulps + 1, dtype=np.int64)[None, :]).reshape(-1)
    return np.unique(p[(p >= 0) & (p < (1 << 32))]).astype(np.uint32)


# ---- libm on the device ----------------------------------------------------------------------------------------------
# the host test's grids (tests/test_libm_restatement.py), and around them: expf's overflow / underflow thresholds
# (88.72, -103.97 = result 0, -103.28 = the last subnormal results; the |x| >= 88 special-case entry) and logf's subnormals
EXPF_GRIDS = [SWEEP, (0xC0000000, 0xC2800000, 1), (0x42AF0000, 0x42B30000, 1), (0xC2AF0000, 0xC2D10000, 1)]
LOGF_GRIDS = [SWEEP, (0x3F000000, 0x40000000, 1), (0x00000000, 0x00810000, 1)]
LOG_SEED, LOG_POINTS = 0xC0FFEE, 4_000_000


@pytest.fixture(scope="module")
def glibc_referees():
    """The live glibc is the referee only if the HOST compile of the restatement agrees with it on the very grids used
    below.  (A device mismatch never skips.)"""
    L = U.libm_check()
    for name, grids in (("cmp_expf", EXPF_GRIDS), ("cmp_logf", LOGF_GRIDS)):
        def one(g, name=name):
            return getattr(L, name)(g[0], g[1], g[2], None)
        pieces = [(lo, lo + n * g[2], g[2]) for g in grids for lo, n in U.range_chunks(*g)]
        if sum(U.in_threads(one, pieces)):
            pytest.skip(f"host restatement differs from this machine's libm ({name}): its glibc is not the 2.35 FMA variant, no referee")
    bad64 = C.c_uint64(0)
    if L.cmp_log(LOG_SEED, LOG_POINTS, C.byref(bad64)):
        pytest.skip("host restatement differs from this machine's libm (log): its glibc is not the 2.35 FMA variant, no referee")
    return L


@pytest.mark.parametrize("name,fn,ref,grids", [("ulcx_expf", UF_EXPF, 0, EXPF_GRIDS), ("ulcx_expf_t (LDS table)", UF_EXPF_T, 0, EXPF_GRIDS),
                                               ("ulcx_logf", UF_LOGF, 1, LOGF_GRIDS)], ids=["expf", "expf_t", "logf"])
def test_libm_f32_on_device(glibc_referees, name, fn, ref, grids):
    L = glibc_referees
    for g in grids:
        pieces = U.range_chunks(*g)
        got = [U.dev_f32(fn, n, lo=lo, stride=g[2]) for lo, n in pieces]

        def check(i):
            bad, want = C.c_uint32(0), C.c_uint32(0)
            m = L.cmp_f32_arr(ref, ptr(got[i]), None, pieces[i][0], g[2], pieces[i][1], C.byref(bad), C.byref(want))
            return m, bad.value, want.value, i
        res = U.in_threads(check, range(len(pieces)))
        total = sum(r[0] for r in res)
        first = next((r for r in res if r[0]), None)
        if first:
            x = first[1]
            k = (x - pieces[first[3]][0]) // g[2]
            assert total == 0, (f"{name}: {total} mismatches on the grid {g[0]:#x}..{g[1]:#x} step {g[2]}, first at argument {x:#010x} "
                                f"({f32(x)!r}): device {got[first[3]][k]:#010x}, glibc {first[2]:#010x}")


def test_libm_log_f64_on_device(glibc_referees):
    L = glibc_referees
    x = np.empty(LOG_POINTS, np.uint64)
    L.gen_log_inputs(LOG_SEED, LOG_POINTS, ptr(x))
    # the four regimes of cmp_log: any positive finite, [0.5, 2), values that come from binary32, subnormals
    assert (x[1::4] >= 0x3FE0000000000000).all() and (x[1::4] < 0x4000000000000000).all() and (x[3::4] < 0x0010000000000000).all()
    got = U.dev_log(x)
    bad, want = C.c_uint64(0), C.c_uint64(0)
    m = L.cmp_log_arr(ptr(got), ptr(x), LOG_POINTS, C.byref(bad), C.byref(want))
    if m:
        i = int(np.flatnonzero(x == bad.value)[0])
        assert m == 0, f"ulcx_log: {m} mismatches, first at argument {bad.value:#018x}: device {int(got[i]):#018x}, glibc {want.value:#018x}"


# ---- scalar helpers against the oracle -------------------------------------------------------------------------------
QUANT_UNDEF = (0x5E800000, 0x7F800000)         # 2^62 .. +inf: 0.5f + sqrtf(v - 0.25f) >= 2^31


def _quant_steps():
    q = np.arange(0, 18, dtype=np.float64)
    # q^2 - q + 0.25 = (q - 0.5)^2 is where sqrtf's ARGUMENT crosses a step, q^2 - q + 0.5 where v does; both, and 0.5 (the
    # entry test) - through q = 17 so that the clamp at 16 has values on both sides
    return np.concatenate([q * q - q + 0.25, q * q - q + 0.5, [0.5, 0.25]]).astype(np.float32)


def _dense_patterns(fn):
    if fn in (UF_QUANT_U, UF_QUANT_COEF_U):
        return around(_quant_steps(), 64)
    if fn == UF_QUANT_COEF:
        s = _quant_steps()
        return around(np.concatenate([s, -s]), 64)
    if fn == UF_BUILD_QUANTIZER:
        # class boundaries: 0x1.657006p2 - 0x1.715476p0 * ln(maxv) = k, for every k the clamp to 5..31 can see and a few beyond;
        # logf's rounding moves a boundary by a few ulps at most: 4096 each side
        k = np.arange(2, 36, dtype=np.float64)
        v = np.exp((float.fromhex("0x1.657006p2") - k) / float.fromhex("0x1.715476p0"))
        return around(v.astype(np.float32), 4096)
    if fn == UF_TO_PCM16:
        k = np.arange(-32770, 32770, dtype=np.float64)
        ties = ((k + 0.5) / 32768.0).astype(np.float32)                    # exact: k + 0.5 has 17 significant bits
        assert (ties.astype(np.float64) * 32768.0 == k + 0.5).all()
        return np.union1d(around(ties, 1), around(np.array([1.0, -1.0, 32767.0 / 32768.0, -32767.0 / 32768.0], np.float32), 4096))
    if fn == UF_FASTLOG:
        return around(np.array([1.0, 2.0, 0.5, 2.0 ** -126, 2.0 ** -31], np.float32), 4096)
    raise AssertionError(fn)


def _undefined_ranges(fn):
    """pattern intervals [a, b] outside the C reference's domain (module docstring)"""
    if fn in (UF_QUANT_U, UF_QUANT_COEF_U):
        return [QUANT_UNDEF]
    if fn == UF_QUANT_COEF:
        return [QUANT_UNDEF, (QUANT_UNDEF[0] | 0x80000000, QUANT_UNDEF[1] | 0x80000000)]
    if fn == UF_BUILD_QUANTIZER:
        return [(0, 0), (0x7F800000, 0xFFFFFFFF)]                          # +0; +inf, NaN and everything with the sign bit
    if fn == UF_TO_PCM16:
        return [(0x7F800000, 0x7FFFFFFF), (0xFF800000, 0xFFFFFFFF)]        # +-inf, NaN
    return []


def test_quantiser_domain_edge_is_two_to_the_62():
    """the interval QUANT_UNDEF, from binary32 arithmetic alone (numpy's sqrt is correctly rounded)"""
    edge = f32(np.array([QUANT_UNDEF[0] - 1, QUANT_UNDEF[0]], np.uint32))
    r = np.float32(0.5) + np.sqrt(edge - np.float32(0.25))
    assert r.dtype == np.float32 and r[0] < np.float32(2.0 ** 31) and r[1] >= np.float32(2.0 ** 31)


SCALAR_CASES = [("fastlog", UF_FASTLOG, 0), ("quant_u", UF_QUANT_U, 0)] + \
               [("quant_coef_u", UF_QUANT_COEF_U, lim) for lim in (7, 8, 16)] + [("quant_coef", UF_QUANT_COEF, lim) for lim in (7, 8, 16)] + \
               [("build_quantizer", UF_BUILD_QUANTIZER, 0), ("to_pcm16", UF_TO_PCM16, 0)]


@pytest.mark.parametrize("name,fn,arg", SCALAR_CASES, ids=[f"{c[0]}-{c[2]}" if c[2] else c[0] for c in SCALAR_CASES])
def test_scalar_helper_on_device_against_oracle(name, fn, arg):
    R = U.units_ref()
    undefined = _undefined_ranges(fn)

    def compare(got, patterns, lo, stride, n):
        bad, want, skipped = C.c_uint32(0), C.c_uint32(0), C.c_longlong(0)
        m = R.ref_cmp_f32(fn, arg, ptr(got), ptr(patterns) if patterns is not None else None, lo, stride, n,
                          C.byref(bad), C.byref(want), C.byref(skipped))
        assert m >= 0
        return m, bad.value, want.value, skipped.value

    def report(m, bad, want, got_at, where):
        shown = (lambda v: f"{v:#010x} ({f32(v)!r})") if fn == UF_FASTLOG else (lambda v: str(int(v) - (1 << 32) if int(v) >= (1 << 31) else int(v)))
        return (f"{name}{f' limit {arg}' if arg else ''}: {m} mismatches {where}, first at argument {bad:#010x} ({f32(bad)!r}): "
                f"device {shown(got_at)}, oracle {shown(want)}")

    # 1. the strided sweep of all binary32 patterns
    lo0, hi0, stride = SWEEP
    pieces = U.range_chunks(lo0, hi0, stride)
    got = [U.dev_f32(fn, n, arg=arg, lo=lo, stride=stride) for lo, n in pieces]
    res = U.in_threads(lambda i: compare(got[i], None, pieces[i][0], stride, pieces[i][1]), range(len(pieces)))
    for i, (m, bad, want, _) in enumerate(res):
        if m:
            total = sum(r[0] for r in res)
            assert total == 0, report(total, bad, want, got[i][(bad - pieces[i][0]) // stride], "on the stride-61 sweep")
    outside = sum(U.count_in(a, b, lo0, hi0, stride) for a, b in undefined)
    assert sum(r[3] for r in res) == outside, f"{name}: the referee left out {sum(r[3] for r in res)} points of the sweep, {outside} lie outside its domain"

    # 2. dense around the places where the result changes
    pat = _dense_patterns(fn)
    gd = U.dev_f32(fn, pat.size, arg=arg, patterns=pat)
    m, bad, want, skipped = compare(gd, pat, 0, 0, pat.size)
    if m:
        assert m == 0, report(m, bad, want, gd[int(np.flatnonzero(pat == bad)[0])], "on the dense ranges")
    outside = sum(int(((pat >= a) & (pat <= b)).sum()) for a, b in undefined)
    assert skipped == outside, f"{name}: the referee left out {skipped} points of the dense ranges, {outside} lie outside its domain"


def test_expand_quantizer_on_device():
    """q = 0..31 (30: the index decode_code gives a unit that opens with Fh - a corrupt stream): 2^-(5+q) while the reference's
    (1u << 26) >> q has a bit left, 0.0 from q = 27 on (ulcDecoder.c:96-98)"""
    q = np.arange(32, dtype=np.uint32)
    got = f32(U.dev_f32(UF_EXPAND_QUANTIZER, q.size, patterns=q))
    want = np.where(q <= 26, np.ldexp(1.0, -(5 + q.astype(np.int64))), 0.0).astype(np.float32)
    assert bits_of(want[30]) == 0 and bits_of(want[26]) == bits_of(np.float32(2.0 ** -31))
    bad = np.flatnonzero(bits_of(got) != bits_of(want))
    assert bad.size == 0, f"expand_quantizer: first mismatch at q = {bad[0]}: device {got[bad[0]]!r}, reference {want[bad[0]]!r}"


# ---- sel_key ---------------------------------------------------------------------------------------------------------
HALF_EPS = 0x2F800000                  # 0.5 * ULCX_COEF_EPS = 2^-32


def _sel_key_inputs():
    rng = np.random.default_rng(20240611)
    sweep = np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                        0x3F800000, 0xBF800000, 0x7F7FFFFF, 0xFF7FFFFF], np.uint32)
    edge = np.concatenate([around(f32(np.array([HALF_EPS, HALF_EPS | 0x80000000], np.uint32)), 8), around(np.array([2.0 ** -31, -2.0 ** -31], np.float32), 8)])
    re = np.unique(np.concatenate([sweep, special, edge]))
    chan = np.float32(float.fromhex("-0x1.62E430p0"))
    fixed = np.array([0.0, 0.0, -0.0, -np.inf, chan, -chan], np.float32)   # (column 0 is replaced on the device: -2 * fastlog(re^2))
    m = np.concatenate([fixed, rng.uniform(-60.0, 20.0, 256 - fixed.size).astype(np.float32)])
    return re, bits_of(m)


@pytest.mark.parametrize("ch", [0, 1])
def test_sel_key_equals_the_ordered_final_key(ch):
    re, m = _sel_key_inputs()
    assert np.isin([0, 0x80000000, 1, HALF_EPS - 1, HALF_EPS, HALF_EPS + 1], re).all() and m.size == 256
    sel, ref = U.dev_sel_key(re, m, True, ch)
    bad = np.argwhere(sel != ref)
    if bad.size:
        i, j = bad[0]
        lvl = "-2 * fastlog(re^2)" if j == 0 else f"{m[j]:#010x} ({f32(m[j])!r})"
        assert False, (f"sel_key != key_ord(final_key(key0_of(re), m, ch)) at {bad.shape[0]} inputs (ch = {ch}), first: re {re[i]:#010x} ({f32(re[i])!r}), "
                       f"m {lvl}: sel_key {sel[i, j]:#010x}, ordered final key {ref[i, j]:#010x}")


def test_key_ord_is_strictly_monotone_in_the_float_order():
    lo0, hi0, stride = SWEEP
    for lo, n in U.range_chunks(lo0, hi0 - 1, stride):
        a = (lo + stride * np.arange(n, dtype=np.uint64)).astype(np.uint32)
        ka, kb = U.dev_f32(UF_KEY_ORD, n, lo=lo, stride=stride), U.dev_f32(UF_KEY_ORD, n, lo=lo + 1, stride=stride)
        fa, fb = f32(a), f32(a + np.uint32(1))
        ok = np.isnan(fa) | np.isnan(fb)                                      # no order among NaN
        with np.errstate(invalid="ignore"):
            ok |= ((fa < fb) & (ka < kb)) | ((fa > fb) & (ka > kb)) | ((fa == fb) & (ka == kb))
        bad = np.flatnonzero(~ok)
        assert bad.size == 0, (f"key_ord: order of the adjacent patterns {a[bad[0]]:#010x} / +1 ({fa[bad[0]]!r}, {fb[bad[0]]!r}) "
                               f"not kept: keys {ka[bad[0]]:#010x}, {kb[bad[0]]:#010x}")
    z = U.dev_f32(UF_KEY_ORD, 6, patterns=np.array([0x80000000, 0x00000000, 0x80000001, 0x00000001, 0xFF800000, 0x7F800000], np.uint32))
    assert z[0] == z[1], "key_ord: -0 and +0 must map to one key"
    assert z[4] < z[2] < z[0] < z[3] < z[5], "key_ord: -inf < -tiny < 0 < +tiny < +inf"


# ---- decode_code: all 2^20 windows x first ---------------------------------------------------------------------------
# fields compared per kind of code (the others are don't-care: the walk never reads them for that kind)
#   every kind      len, plain, zrun, n8, tail, stop, qnew (-1 unless the code sets a quantizer), n and np (the walk adds
#                   both for every code: n = 1 plain / the run of a zero run / else 0, np = the run of a noise run / else 0)
#   plain           sv
#   noise run       l
#   tail            l, dn
ALWAYS = ("len", "plain", "zrun", "n8", "tail", "stop", "qnew", "n", "np")


def _decode_code_reference(w, first):
    """Branch cascade from the code table (FormatSpecs.md:60-71 / the comment in front of decode_code, ulcDecoder.c:99-197) over an
    array of windows.  -> dict of int arrays per field, and `kind`."""
    w = w.astype(np.int64)
    ny = [(w >> (4 * k)) & 15 for k in range(5)]
    if first:
        v = [np.full_like(w, 0xF)] + ny[:4]              # a unit's opening quantizer code: "akin to a silent Fh"
    else:
        v = ny
    z = np.zeros_like(w)
    out = {f: z.copy() for f in CODE_FIELDS}
    out["qnew"] -= 1
    v0, v1, v2, v3, v4 = v
    is_zs, is_zl, is_n8, is_esc = v0 == 0x0, v0 == 0x1, v0 == 0x8, v0 == 0xF
    is_plain = ~(is_zs | is_zl | is_n8 | is_esc)
    is_q = is_esc & (v1 <= 0xD)
    is_qx = is_esc & (v1 == 0xE) & (v2 != 0xF)
    is_stop = is_esc & (v1 == 0xE) & (v2 == 0xF)
    is_tail = is_esc & (v1 == 0xF)
    opening_f = np.zeros_like(is_esc)
    if first:
        # Fh where the opening quantizer should be: no tail (there is no quantizer yet) - the reference expands "quantizer -2",
        # a shift by 30 on x86-64: quantizer 0.0 = index 30, one nybble read
        opening_f, is_tail = is_tail, np.zeros_like(is_tail)
    s = np.where(v0 >= 8, v0 - 16, v0)
    for mask, fields in ((is_plain, dict(plain=1, len=1, n=1, sv=s * np.abs(s))),
                         (is_zs, dict(zrun=1, len=2, n=v1 + 1)),
                         (is_zl, dict(zrun=1, len=3, n=((v1 << 4) | v2) + 33)),
                         (is_n8, dict(n8=1, len=4, np=((((v1 << 4) | v2) << 1) | (v3 & 1)) + 16, l=(v3 >> 1) + 1)),
                         (is_q, dict(len=2, qnew=v1)),
                         (is_qx, dict(len=3, qnew=0xE + v2)),
                         (is_stop, dict(stop=1, len=3)),
                         (is_tail, dict(tail=1, len=5, l=v2 + 1, dn=(v3 << 4) | v4)),
                         (opening_f, dict(len=2, qnew=30))):
        for f, val in fields.items():
            out[f] = np.where(mask, val, out[f])
    if first:
        out["len"] = out["len"] - 1                       # the silent Fh is not in the stream
    kinds = dict(plain=is_plain, noise_run=is_n8, tail=is_tail)
    assert ((is_plain.astype(int) + is_zs + is_zl + is_n8 + is_q + is_qx + is_stop + is_tail + opening_f) == 1).all()
    return out, kinds


@pytest.mark.parametrize("first", [0, 1])
def test_decode_code_exhaustive(first):
    n = 1 << 20
    got = U.dev_decode_code(0, n, first)
    w = np.arange(n, dtype=np.int64)
    ref, kinds = _decode_code_reference(w, first)
    compared = [(f, np.ones(n, bool)) for f in ALWAYS] + [("sv", kinds["plain"]), ("l", kinds["noise_run"] | kinds["tail"]), ("dn", kinds["tail"])]
    for f, where in compared:
        g = got[:, CODE_FIELDS.index(f)].astype(np.int64)
        bad = np.flatnonzero(where & (g != ref[f]))
        assert bad.size == 0, (f"decode_code(first = {first}): field `{f}` differs for {bad.size} windows, first {int(w[bad[0]]):#07x} "
                               f"(nybbles low first: {' '.join(format((int(w[bad[0]]) >> (4 * k)) & 15, 'X') for k in range(5))}): "
                               f"device {g[bad[0]]}, code table {ref[f][bad[0]]}")


# ---- plain_prefix: all 2^28 seven-nybble windows, the eighth nybble 0h and 5h -----------------------------------------
@pytest.mark.parametrize("top", [0x0, 0x5])
def test_plain_prefix_exhaustive(top):
    R = U.units_ref()
    chunk = 1 << 26
    los = list(range(0, 1 << 28, chunk))
    got = [U.dev_plain_prefix(lo, top, chunk) for lo in los]                  # 64 MB each on the device

    def check(i):
        parts = 4
        out = []
        for p in range(parts):                                                # (four pieces per chunk: sixteen referee calls on the threads)
            bad, want = C.c_uint32(0), C.c_int(0)
            off = p * (chunk // parts)
            m = R.ref_cmp_plain_prefix(ptr(got[i][off:]), los[i] + off, top, chunk // parts, C.byref(bad), C.byref(want))
            out.append((m, bad.value, want.value))
        return out
    res = [r for rs in U.in_threads(check, range(len(los))) for r in rs]
    total = sum(r[0] for r in res)
    first = next((r for r in res if r[0]), None)
    if first:
        wbad = first[1]
        g = got[(wbad & 0x0FFFFFFF) // chunk][(wbad & 0x0FFFFFFF) % chunk]
        assert total == 0, f"plain_prefix: {total} windows differ (eighth nybble {top:X}h), first {wbad:#010x}: device {g}, the loop {first[2]}"
    # the referee itself on a few windows by hand: 2..7 / 9..E are plain, 0 1 8 F stop the run, seven nybbles at most
    for wv, want in ((0x02345670, 0), (0x0234567F, 0), (0x01234562, 6), (0x0EDCBA92, 7), (0x08222222, 6), (0x0222222F, 0)):
        bad, wnt = C.c_uint32(0), C.c_int(0)
        R.ref_cmp_plain_prefix(ptr(np.array([255], np.uint8)), wv, 0, 1, C.byref(bad), C.byref(wnt))
        assert wnt.value == want, hex(wv)


# ---- rng_jump --------------------------------------------------------------------------------------------------------
def _rng_states():
    rng = np.random.default_rng(75)
    return np.concatenate([np.array([0, 1, 1234567, 0xFFFFFFFF], np.uint32), rng.integers(0, 1 << 32, 1000, dtype=np.uint64).astype(np.uint32)])


def _gf2_apply(cols, v):
    """matrix (32 columns, uint32 each) times every vector of the array v, over GF(2)"""
    r = np.zeros_like(v)
    for b in range(32):
        r ^= np.where((v >> np.uint32(b)) & np.uint32(1), cols[b], np.uint32(0)).astype(np.uint32)
    return r


def _xorshift_powers():
    """T^(2^j), j < 32, T = one step of the generator (ulcDecoder.c:75-81), each as its 32 columns"""
    s = (np.uint32(1) << np.arange(32, dtype=np.uint32)).astype(np.uint32)
    s ^= s << np.uint32(13)
    s ^= s >> np.uint32(17)
    s ^= s << np.uint32(5)
    pw = [s]
    for _ in range(31):
        pw.append(_gf2_apply(pw[-1], pw[-1]))                                  # columns of A*A = A applied to the columns of A
    return pw


def test_rng_jump_contiguous_lengths_against_the_iterated_generator():
    R = U.units_ref()
    states, nlen = _rng_states(), 70001
    lengths = np.arange(nlen, dtype=np.uint32)
    groups = [states[i:i + 251] for i in range(0, states.size, 251)]            # 70 MB of results each
    got = [U.dev_rng_jump(g, lengths) for g in groups]

    def check(i):
        bad, want = (C.c_longlong * 2)(0, 0), C.c_uint32(0)
        m = R.ref_cmp_rng_iter(ptr(got[i]), ptr(groups[i]), groups[i].size, nlen, bad, C.byref(want))
        return m, bad[0], bad[1], want.value
    for i, (m, si, k, want) in enumerate(U.in_threads(check, range(len(groups)))):
        assert m == 0, (f"rng_jump: {m} results differ from orc_xorshift32 iterated, first: state {int(groups[i][si]):#010x}, length {k}: "
                        f"device {int(got[i][si, k]):#010x}, iterated {want:#010x}")


def _long_lengths():
    rng = np.random.default_rng(76)
    cells = [d * 16 ** i for i in range(8) for d in range(1, 16)]              # one table cell each
    borrow = [16 ** i - 1 for i in range(9)]                                   # every lower digit Fh; 16^8 - 1 = 2^32 - 1
    return np.unique(np.array(cells + borrow + [0, 70000, 70001, (1 << 32) - 1] + list(rng.integers(0, 1 << 32, 300, dtype=np.uint64)), np.uint64)).astype(np.uint32)


def test_rng_jump_long_lengths_against_matrix_powers():
    states, lengths = _rng_states(), _long_lengths()
    assert {15 * 16 ** 7, 16 ** 7, (1 << 32) - 1}.issubset(set(int(x) for x in lengths))
    got = U.dev_rng_jump(states, lengths)
    pw = _xorshift_powers()
    want = np.repeat(states[None, :], lengths.size, 0)                          # [length][state]
    for j in range(32):
        rows = np.flatnonzero((lengths >> np.uint32(j)) & np.uint32(1))
        if rows.size:
            want[rows] = _gf2_apply(pw[j], want[rows])
    bad = np.argwhere(got != want.T)
    if bad.size:
        si, li = bad[0]
        assert False, (f"rng_jump: {bad.shape[0]} results differ from T^n by square-and-multiply, first: state {int(states[si]):#010x}, "
                       f"length {int(lengths[li])} ({int(lengths[li]):#x}): device {int(got[si, li]):#010x}, matrix power {int(want[li, si]):#010x}")


def test_rng_jump_is_additive():
    rng = np.random.default_rng(77)
    n = 200_000
    s = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    s[:4] = [0, 1, 1234567, 0xFFFFFFFF]
    a = rng.integers(0, 1 << 31, n, dtype=np.uint64)
    b = rng.integers(0, 1 << 31, n, dtype=np.uint64)
    a[n // 2:] >>= rng.integers(0, 31, n - n // 2).astype(np.uint64)           # short and long pieces mixed
    assert (a + b < (1 << 32)).all()
    two = U.dev_rng_jump_each(U.dev_rng_jump_each(s, a.astype(np.uint32)), b.astype(np.uint32))
    one = U.dev_rng_jump_each(s, (a + b).astype(np.uint32))
    bad = np.flatnonzero(two != one)
    assert bad.size == 0, (f"rng_jump: jump(jump(s, a), b) != jump(s, a + b) for {bad.size} inputs, first s = {int(s[bad[0]]):#010x}, "
                           f"a = {int(a[bad[0]])}, b = {int(b[bad[0]])}: {int(two[bad[0]]):#010x} vs {int(one[bad[0]]):#010x}")


# ---- wave primitives -------------------------------------------------------------------------------------------------
def _wave_rows():
    rng = np.random.default_rng(78)
    rows = [np.zeros(64, np.uint32), np.full(64, 0xFFFFFFFF, np.uint32)]
    for p in range(64):                                                        # a single non-zero lane
        r = np.zeros(64, np.uint32); r[p] = 0x80000001 + p; rows.append(r)
    rows.append((0xFFFFFF00 - 0x01010101 * np.arange(64, dtype=np.uint64)).astype(np.uint32))          # descending ramp
    rows.append(np.arange(64, 0, -1).astype(np.uint32))
    for p in (0, 15, 16, 31, 32, 63):                                          # the extremum on the row / bank boundaries of the DPP steps
        hi = rng.integers(1000, 1 << 31, 64, dtype=np.uint64).astype(np.uint32); hi[p] = 0xFFFFFFFF; rows.append(hi)
        lo = rng.integers(1000, 1 << 31, 64, dtype=np.uint64).astype(np.uint32); lo[p] = 0; rows.append(lo)
        hi2 = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32); hi2[p] = 0xFFFFFFFF; rows.append(hi2)
    adversarial = np.stack(rows)
    n_rand = 4 * 320 - adversarial.shape[0]                                    # 320 workgroups of four waves in all
    full = rng.integers(0, 1 << 32, (n_rand // 2, 64), dtype=np.uint64).astype(np.uint32)
    small = rng.integers(0, 600, (n_rand - n_rand // 2, 64), dtype=np.uint64).astype(np.uint32)       # sums that do not wrap (draw counts, nybble counts)
    allrows = np.concatenate([adversarial, full, small])
    return allrows[rng.permutation(allrows.shape[0])]                          # unlike rows share a workgroup: a leak between waves shows


def test_wave_primitives_on_device():
    rows = _wave_rows()
    assert rows.shape == (1280, 64) and rows.dtype == np.uint32
    got = U.dev_wave(rows)
    incl = np.cumsum(rows, axis=1, dtype=np.uint32)
    total = rows.sum(axis=1, dtype=np.uint32)
    assert (incl[:, 63] == total).all() and (total[(rows == 0xFFFFFFFF).all(1)] == np.uint32(-64 & 0xFFFFFFFF)).all()
    every = lambda v: np.repeat(v[:, None], 64, 1)                             # a reduction's result is in every lane
    want = [every(total), every(rows.min(axis=1)), every(rows.max(axis=1)), incl, np.maximum.accumulate(rows, axis=1),
            incl - rows, every(total)]
    failures = []
    for k, name in enumerate(U.WAVE_PLANES):
        bad = np.argwhere(got[k] != want[k])
        if bad.size:
            r, lane = bad[0]
            failures.append(f"{name}: {bad.shape[0]} lanes differ, first: row {r} (wave {r % 4} of workgroup {r // 4}) lane {lane}: device {int(got[k][r, lane]):#010x}, "
                            f"numpy {int(want[k][r, lane]):#010x}; the row: {' '.join(format(int(x), 'x') for x in rows[r])}")
    assert not failures, "\n".join(failures)


# ---- noise_q_from_sums / hfext_from_sums -----------------------------------------------------------------------------
def _noise_cases():
    """-> pairs [total][2] {w, w * logNoise}, off, cnt, q per case"""
    rng = np.random.default_rng(79)
    logs, qs = [], []

    def add(level, q=None):
        logs.append(np.clip(np.asarray(level, np.float64), -40.0, 5.0))
        qs.append(float(1 << int(rng.integers(5, 32))) if q is None else q)      # the writer's (float)(1u << quantizer index), index 5..31
    for _ in range(3000):                                                         # general: a line with jitter, 1..64 pairs
        n = int(rng.integers(1, 65))
        add(rng.uniform(-40, 5) + rng.uniform(-0.6, 0.3) * np.arange(n) + rng.normal(0, rng.uniform(0, 3), n))
    for n in range(1, 65):                                                        # every count once more, flat spectrum (decay ~ 1)
        add(rng.uniform(-40, 5, n))
    for _ in range(200):                                                          # a single pair: det == 0
        add([rng.uniform(-40, 5)])
    for _ in range(200):                                                          # positive slope: decay clamps to 1, outputs untouched
        n = int(rng.integers(2, 65)); add(-38 + rng.uniform(0.05, 0.6) * np.arange(n))
    for _ in range(200):                                                          # steep: decay quantises above FFh
        n = int(rng.integers(2, 65)); add(5 - rng.uniform(0.3, 0.7) * np.arange(n))
    for k in range(5, 32):                                                        # every quantiser scale on one spectrum
        add(-3.0 - 0.05 * np.arange(40), q=float(1 << k))
    cnt = np.array([l.size for l in logs], np.int32)
    off = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int32)
    lv = np.concatenate(logs).astype(np.float32)
    w = np.exp(np.float32(0.5) * lv).astype(np.float32)
    pairs = np.stack([w, w * lv], 1).astype(np.float32)
    zero = [i for i in range(0, 3000, 150)]                                       # all-zero weights: sum == 0, det == 0
    for i in zero:
        pairs[off[i]:off[i] + cnt[i]] = 0.0
    return np.ascontiguousarray(pairs), off, cnt, np.array(qs, np.float32), zero


@pytest.fixture(scope="module")
def noise_cases():
    """the cases, the sums the device functions take (host, binary32, the kernels' order) and the oracle's answers - computed once"""
    R = U.units_ref()
    pairs, off, cnt, q, zero = _noise_cases()
    n = q.size
    assert int(off[-1]) + int(cnt[-1]) == pairs.shape[0] and cnt.min() == 1 and cnt.max() == 64
    sum2, sum5 = np.empty((n, 2), np.float32), np.empty((n, 5), np.float32)
    refq, refhf = np.empty(n, np.int32), np.empty((n, 2), np.int32)
    R.ref_noise_cases(ptr(pairs), ptr(off), ptr(cnt), ptr(q), n, ptr(sum2), ptr(sum5), ptr(refq), ptr(refhf))
    # the degenerate classes are there, and the domain: every amplitude the oracle converted fits an int by far
    det = sum5[:, 4] * sum5[:, 1] - sum5[:, 0] * sum5[:, 0]
    assert (det[zero] == 0).all() and (sum2[zero, 0] == 0).all() and (det[cnt == 1] == 0).all()
    assert (refhf[:, 1] == 0xFF).sum() >= 100 and ((refhf[:, 1] == 0) & (det != 0)).sum() >= 100 and (refhf[:, 1] > 0).sum() >= 1000
    assert np.isfinite(sum2).all() and np.isfinite(sum5).all() and refq.min() >= 0 and refq.max() <= 8 and refhf.min() >= 0 and refhf[:, 0].max() <= 16
    for a in (cnt, q, sum2, sum5, refq, refhf):
        a.setflags(write=False)
    return cnt, q, sum2, sum5, refq, refhf


def test_noise_q_from_sums_on_device(noise_cases):
    cnt, q, sum2, _, refq, _ = noise_cases
    gq = U.dev_noise_q(sum2, q)
    bad = np.flatnonzero(gq != refq)
    assert bad.size == 0, (f"noise_q_from_sums: {bad.size} of {q.size} cases differ from orc_get_noise_q, first case {bad[0]} ({cnt[bad[0]]} pairs, q = {q[bad[0]]!r}, "
                           f"sum {sum2[bad[0], 0]!r} ({bits_of(sum2[bad[0], 0]):#010x}), sumw {sum2[bad[0], 1]!r} ({bits_of(sum2[bad[0], 1]):#010x})): device {gq[bad[0]]}, oracle {refq[bad[0]]}")


def test_hfext_from_sums_on_device(noise_cases):
    cnt, q, _, sum5, _, refhf = noise_cases
    gh = U.dev_hfext(sum5, q)
    bad = np.flatnonzero((gh != refhf).any(1))
    assert bad.size == 0, (f"hfext_from_sums: {bad.size} of {q.size} cases differ from orc_get_hfext_params, first case {bad[0]} ({cnt[bad[0]]} pairs, q = {q[bad[0]]!r}, "
                           f"sums {[f'{x!r} ({bits_of(x):#010x})' for x in sum5[bad[0]]]}): device {{NoiseQ, NoiseDecay}} = {gh[bad[0]].tolist()}, oracle {refhf[bad[0]].tolist()}")


# ---- the view of a corpus --------------------------------------------------------------------------------------------
# corpus_file / file_block (ulcx_dec_dev.h): what every indexed walk and the splice kernels read a corpus through.  The model is
# the rule as include/ulc_amd.h states it, in Python integers; the tables hold every hostile case once.  Nothing is decoded and no
# payload byte exists: the offsets are arithmetic only (one file is exactly 2^31 bytes long).
VIEW_KS = (-1, 0, 1, 2, 3, 4, 5)


def _view_model(byte_offs, index_blocks, pay_offs=None, idx_offs=None, pay_total=0, pay_stride=0, pay_bytes=None, index_stride=0):
    rows = []
    for f, nb in enumerate(int(x) for x in index_blocks):
        if pay_offs is not None:
            p0, p1, i0, i1 = int(pay_offs[f]), int(pay_offs[f + 1]), int(idx_offs[f]), int(idx_offs[f + 1])
            ok = 0 <= p0 <= p1 <= pay_total and p1 - p0 < 2 ** 31 and 0 <= i0 <= i1 <= len(byte_offs) and i1 - i0 >= max(nb, 0) + 1
            base, row, avail, nI = (p0, i0, p1 - p0, max(nb, 0)) if ok else (0, 0, 0, 0)
        else:
            base, row = f * pay_stride, f * index_stride
            avail, nI = min(max(int(pay_bytes[f]), 0), pay_stride), min(max(nb, 0), index_stride - 1)
        out = [base, row, avail, nI]
        for k in VIEW_KS:
            off = ext = 0
            if 0 <= k < nI:
                o0, o1 = int(byte_offs[row + k]), int(byte_offs[row + k + 1])
                if o0 >= 0 and o0 < o1 <= avail:
                    off, ext = o0, o1 - o0
            out += [off, ext]
        rows.append(out)
    return np.array(rows, np.int64)


_G = 2 ** 31
VIEW_CORPORA = {
    # rows of 6 entries, payloads 1000 bytes apart
    "strided": dict(pay_stride=1000, index_stride=6,
                    #            sound  count < 0  count > stride-1  bytes < 0  bytes > stride  falling entry  entry < 0  entries past the bytes / equal
                    index_blocks=[4,    -3,        9,                2,         3,              3,             2,         4],
                    pay_bytes=[900,     500,       60,               -5,        5000,           1000,          1000,      150],
                    byte_offs=[0, 100, 250, 400, 900, -1,   0, 10, 20, -1, -1, -1,   0, 10, 20, 30, 40, 50,   0, 10, 20, -1, -1, -1,
                               0, 500, 1000, 1200, -1, -1,   0, 300, 200, 400, -1, -1,   -4, 100, 200, -1, -1, -1,   0, 100, 100, 200, 120, -1]),
    # hostile payload offsets: a pair that falls into a negative entry, a negative start, a falling pair, a file of exactly 2^31
    # bytes, an end past the total; among the sound files one whose row is one entry short and one whose entries fall / leave it
    "ragged, payload table": dict(pay_total=_G + 5000, pay_offs=[0, 900, -8, 1000, 3000, 2000, 2000 + _G, _G + 4000, _G + 9000],
                                  idx_offs=[0, 5, 5, 10, 14, 14, 20, 26, 30], index_blocks=[4, 0, 2, 4, 0, 3, 4, 2],
                                  byte_offs=[0, 100, 250, 400, 900,   0, 10, 20, 30, 40,   0, 500, 1000, 2000,   0, 10, 20, 30, 40, 50,
                                             0, 500, 400, 2500, 1900, 2000,   0, 10, 20, 30]),
    # hostile index offsets: a falling pair, a negative start, an end and a start past the total; a count < 0
    "ragged, index table": dict(pay_total=800, pay_offs=[0, 100, 200, 300, 400, 500, 600, 700, 800],
                                idx_offs=[0, 4, -2, 8, 6, 12, 16, 40, 20], index_blocks=[-1, 1, 1, 1, 5, 3, 2, 2],
                                byte_offs=[0, 10, 20, 30,   0, 50, 100, -1,   0, 20, 40, 60,   80, 100, 0, 30, 60, 100,   0, 1, 2, 3, 4, 5]),
}


@pytest.mark.parametrize("name", list(VIEW_CORPORA))
def test_corpus_view_on_device(name):
    c = VIEW_CORPORA[name]
    want = _view_model(**c)
    got = U.dev_corpus_view(ks=VIEW_KS, **c)
    assert (want[:, 5::2] > 0).any() and (want[:, 3] == 0).any(), "the tables hold neither a block that is found nor a file without blocks"
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, (f"corpus_file / file_block, {name} corpus: {bad.size} of {len(want)} files differ, first file {bad[0]}: device "
                           f"{{base, row, avail, nI, (off, ext) of blocks {VIEW_KS}}} = {got[bad[0]].tolist()}, model {want[bad[0]].tolist()}")
