"""Plumbing of tests/test_gpu_units.py: the test-only device module (ulc-codec_amd/libulcx_units.so: thin kernels around
the product's own small device functions), and the two host-side referees under tests/helpers/ - libm_check.cpp (the live
glibc, and the host compile of the libm restatement) and units_ref.c (the oracle's scalar helpers over arrays).

Device buffers are torch tensors; the module's entry points are called through ctypes with their addresses.  Every
wrapper sizes its buffers from the element count it passes, and fails on a non-zero return (launch or synchronise error)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
UNITS_LIB = os.path.join(ROOT, "ulc-codec_amd", "libulcx_units.so")
DEV = "cuda"

u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)

# function numbers of ulcx_units_f32 (ulcx_units.hip)
UF_EXPF, UF_EXPF_T, UF_LOGF, UF_FASTLOG, UF_QUANT_U, UF_QUANT_COEF_U, UF_QUANT_COEF, UF_BUILD_QUANTIZER, UF_TO_PCM16, UF_KEY_ORD, \
    UF_EXPAND_QUANTIZER, UF_COUNT = range(12)
CODE_FIELDS = ("len", "n", "np", "l", "dn", "sv", "qnew", "plain", "zrun", "n8", "tail", "stop")


def _stale(so, *srcs):
    return (not os.path.exists(so)) or max(os.path.getmtime(s) for s in srcs) > os.path.getmtime(so)


_libm = None


def libm_check():
    """tests/helpers/libm_check.so: ulcx_libm.h compiled for the host (g++ -mfma) beside the live libm."""
    global _libm
    if _libm is None:
        src = os.path.join(HERE, "helpers", "libm_check.cpp")
        so = os.path.join(HERE, "helpers", "libm_check.so")
        hdr = os.path.join(ROOT, "ulc-codec_amd", "csrc", "ulcx_libm.h")
        if _stale(so, src, hdr):
            subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fPIC", "-shared", "-o", so, src, "-lm"])
        l = C.CDLL(so)
        for f in (l.cmp_expf, l.cmp_logf):
            f.restype = C.c_longlong
            f.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, u32p]
        l.cmp_log.restype = C.c_longlong
        l.cmp_log.argtypes = [C.c_uint64, C.c_longlong, u64p]
        l.arr_f32.restype = None
        l.arr_f32.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_longlong, C.c_void_p]
        l.cmp_f32_arr.restype = C.c_longlong
        l.cmp_f32_arr.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_longlong, u32p, u32p]
        l.gen_log_inputs.restype = None
        l.gen_log_inputs.argtypes = [C.c_uint64, C.c_longlong, C.c_void_p]
        l.arr_log.restype = None
        l.arr_log.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
        l.cmp_log_arr.restype = C.c_longlong
        l.cmp_log_arr.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, u64p, u64p]
        _libm = l
    return _libm


_ref = None


def units_ref():
    """tests/helpers/units_ref.so: the oracle's scalar helpers over arrays (linked against oracle/liboracle.so)."""
    global _ref
    if _ref is None:
        from ulc_testlib import build_oracle
        oracle_so = build_oracle()
        src = os.path.join(HERE, "helpers", "units_ref.c")
        so = os.path.join(HERE, "helpers", "units_ref.so")
        if _stale(so, src, os.path.join(ROOT, "oracle", "ulc_oracle.h"), oracle_so):
            subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-fPIC", "-shared", "-o", so, src,
                                   "-L" + os.path.dirname(oracle_so), "-l:liboracle.so", "-Wl,-rpath,$ORIGIN/../../oracle", "-lm"])
        l = C.CDLL(so)
        l.ref_cmp_f32.restype = C.c_longlong
        l.ref_cmp_f32.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_longlong, u32p, u32p,
                                  C.POINTER(C.c_longlong)]
        l.ref_cmp_rng_iter.restype = C.c_longlong
        l.ref_cmp_rng_iter.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_longlong, C.POINTER(C.c_longlong), u32p]
        l.ref_noise_cases.restype = None
        l.ref_noise_cases.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong] + [C.c_void_p] * 4
        l.ref_cmp_plain_prefix.restype = C.c_longlong
        l.ref_cmp_plain_prefix.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_longlong, u32p, C.POINTER(C.c_int)]
        _ref = l
    return _ref


_units = None


def units_lib():
    global _units
    if _units is None:
        if not os.path.exists(UNITS_LIB):
            raise RuntimeError(f"{UNITS_LIB} not built: run `make -C ulc-codec_amd` (or __graft_entry__.build())")
        l = C.CDLL(UNITS_LIB)
        P, LL, I, U32, U64 = C.c_void_p, C.c_longlong, C.c_int, C.c_uint32, C.c_uint64
        l.ulcx_units_f32.argtypes = [I, I, P, U64, U64, LL, P]
        l.ulcx_units_log.argtypes = [P, LL, P]
        l.ulcx_units_decode_code.argtypes = [U32, LL, I, P]
        l.ulcx_units_plain_prefix.argtypes = [U32, U32, LL, P]
        l.ulcx_units_sel_key.argtypes = [P, LL, P, I, I, I, P, P]
        l.ulcx_units_rng_jump.argtypes = [P, LL, P, LL, P]
        l.ulcx_units_rng_jump_each.argtypes = [P, P, LL, P]
        l.ulcx_units_wave.argtypes = [P, LL, P]
        l.ulcx_units_noise_q.argtypes = [P, P, P, LL, P]
        l.ulcx_units_hfext.argtypes = [P, P, LL, P]
        l.ulcx_units_corpus.argtypes = [I, LL, LL, P, P, P, LL, I, P, P, P, I, P]
        assert l.ulcx_units_function_count() == UF_COUNT, "function numbers of ulcx_units.hip and of the tests differ"
        _units = l
    return _units


# ---- device buffers --------------------------------------------------------------------------------------------------
_TORCH_OF = {"uint32": "int32", "uint64": "int64"}      # torch has no arithmetic on unsigned words: same bits, signed dtype


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)      # (torch takes no read-only array)
    t = _TORCH_OF.get(a.dtype.name)
    return torch.from_numpy(a.view(t) if t else a).to(DEV)


def dev_empty(n, dtype):
    import torch
    return torch.empty(int(n), dtype=getattr(torch, _TORCH_OF.get(np.dtype(dtype).name, np.dtype(dtype).name)), device=DEV)


def from_dev(t, dtype):
    return t.cpu().numpy().view(dtype)


def _sync():
    import torch
    torch.cuda.synchronize()


def _run(fn, *args):
    """One entry point: everything queued through torch has finished before it, and its own return covers launch + synchronise."""
    _sync()
    rc = fn(*args)
    assert rc == 0, f"{fn.__name__}: HIP error {rc}"


def dev_f32(fn, n, arg=0, patterns=None, lo=0, stride=1):
    """uint32 results of function `fn` for the patterns of the array, or for lo + i * stride (mod 2^32), i < n."""
    tin = None
    if patterns is not None:
        patterns = np.ascontiguousarray(patterns, np.uint32)
        assert patterns.ndim == 1 and patterns.size == n
        tin = to_dev(patterns)
    out = dev_empty(n, np.uint32)
    _run(units_lib().ulcx_units_f32, fn, arg, tin.data_ptr() if tin is not None else None, lo, stride, n, out.data_ptr())
    return from_dev(out, np.uint32)


def dev_log(bits):
    bits = np.ascontiguousarray(bits, np.uint64)
    tin, out = to_dev(bits), dev_empty(bits.size, np.uint64)
    _run(units_lib().ulcx_units_log, tin.data_ptr(), bits.size, out.data_ptr())
    return from_dev(out, np.uint64)


def dev_decode_code(lo, n, first):
    out = dev_empty(n * len(CODE_FIELDS), np.int32)
    _run(units_lib().ulcx_units_decode_code, lo, n, int(first), out.data_ptr())
    return from_dev(out, np.int32).reshape(n, len(CODE_FIELDS))


def dev_plain_prefix(lo, top, n):
    out = dev_empty(n, np.uint8)
    _run(units_lib().ulcx_units_plain_prefix, lo, top, n, out.data_ptr())
    return from_dev(out, np.uint8)


def dev_sel_key(re_bits, m_bits, mdiag, ch):
    re_bits, m_bits = np.ascontiguousarray(re_bits, np.uint32), np.ascontiguousarray(m_bits, np.uint32)
    n = re_bits.size * m_bits.size
    tre, tm, sel, ref = to_dev(re_bits), to_dev(m_bits), dev_empty(n, np.uint32), dev_empty(n, np.uint32)
    _run(units_lib().ulcx_units_sel_key, tre.data_ptr(), re_bits.size, tm.data_ptr(), m_bits.size, int(mdiag), ch, sel.data_ptr(), ref.data_ptr())
    shape = (re_bits.size, m_bits.size)
    return from_dev(sel, np.uint32).reshape(shape), from_dev(ref, np.uint32).reshape(shape)


def dev_rng_jump(states, lengths):
    """[states][lengths] grid of rng_jump."""
    states, lengths = np.ascontiguousarray(states, np.uint32), np.ascontiguousarray(lengths, np.uint32)
    ts, tl, out = to_dev(states), to_dev(lengths), dev_empty(states.size * lengths.size, np.uint32)
    _run(units_lib().ulcx_units_rng_jump, ts.data_ptr(), states.size, tl.data_ptr(), lengths.size, out.data_ptr())
    return from_dev(out, np.uint32).reshape(states.size, lengths.size)


def dev_rng_jump_each(states, lengths):
    states, lengths = np.ascontiguousarray(states, np.uint32), np.ascontiguousarray(lengths, np.uint32)
    assert states.shape == lengths.shape and states.ndim == 1
    ts, tl, out = to_dev(states), to_dev(lengths), dev_empty(states.size, np.uint32)
    _run(units_lib().ulcx_units_rng_jump_each, ts.data_ptr(), tl.data_ptr(), states.size, out.data_ptr())
    return from_dev(out, np.uint32)


WAVE_PLANES = ("wave_sum_i32", "wave_min_u32", "wave_max_u32", "wave_scan_add", "wave_scan_max", "wave_excl_scan", "wave_excl_scan total")


def dev_wave(rows):
    """rows [R][64] uint32, R a multiple of 4 (workgroups of four waves) -> [7][R][64] in the order of WAVE_PLANES."""
    rows = np.ascontiguousarray(rows, np.uint32)
    assert rows.ndim == 2 and rows.shape[1] == 64 and rows.shape[0] % 4 == 0
    tin, out = to_dev(rows.reshape(-1)), dev_empty(7 * rows.size, np.uint32)
    _run(units_lib().ulcx_units_wave, tin.data_ptr(), rows.size, out.data_ptr())
    return from_dev(out, np.uint32).reshape(7, rows.shape[0], 64)


def dev_noise_q(sum2, q):
    sum2, q = np.ascontiguousarray(sum2, np.float32), np.ascontiguousarray(q, np.float32)
    n = q.size
    assert sum2.shape == (n, 2)
    ts, tw, tq, out = to_dev(sum2[:, 0]), to_dev(sum2[:, 1]), to_dev(q), dev_empty(n, np.int32)
    _run(units_lib().ulcx_units_noise_q, ts.data_ptr(), tw.data_ptr(), tq.data_ptr(), n, out.data_ptr())
    return from_dev(out, np.int32)


def dev_hfext(sum5, q):
    sum5, q = np.ascontiguousarray(sum5, np.float32), np.ascontiguousarray(q, np.float32)
    n = q.size
    assert sum5.shape == (n, 5)
    ts, tq, out = to_dev(sum5.reshape(-1)), to_dev(q), dev_empty(2 * n, np.int32)
    _run(units_lib().ulcx_units_hfext, ts.data_ptr(), tq.data_ptr(), n, out.data_ptr())
    return from_dev(out, np.int32).reshape(n, 2)


def dev_corpus_view(byte_offs, index_blocks, ks, pay_offs=None, idx_offs=None, pay_total=0, pay_stride=0, pay_bytes=None, index_stride=0):
    """corpus_file and file_block over every file of caller-given tables: [nFiles][4 + 2 * len(ks)] int64 =
    {base offset, row offset in entries, avail, nI, then {off, ext} of block ks[j]}.  byte_offs: the ByteOffs of the whole index
    (its RngState words are zeros).  pay_offs / idx_offs given: a ragged corpus of pay_total bytes; else a strided one."""
    byte_offs, index_blocks, ks = (np.ascontiguousarray(a, np.int32) for a in (byte_offs, index_blocks, ks))
    index = np.zeros((byte_offs.size, 2), np.int32)
    index[:, 0] = byte_offs
    n, opt = index_blocks.size, lambda a, dt: None if a is None else to_dev(np.ascontiguousarray(a, dt))
    ti, tb, tk = to_dev(index.reshape(-1)), to_dev(index_blocks), to_dev(ks)
    tpo, tio, tpb = opt(pay_offs, np.int64), opt(idx_offs, np.int64), opt(pay_bytes, np.int32)
    out = dev_empty(n * (4 + 2 * ks.size), np.int64)
    p = lambda t: None if t is None else t.data_ptr()
    _run(units_lib().ulcx_units_corpus, n, pay_total, pay_stride, p(tpb), p(tpo), ti.data_ptr(), byte_offs.size, index_stride, p(tio), tb.data_ptr(),
         tk.data_ptr(), ks.size, out.data_ptr())
    return from_dev(out, np.int64).reshape(n, 4 + 2 * ks.size)


# ---- grids -----------------------------------------------------------------------------------------------------------
def range_chunks(lo, hi, stride, chunk=1 << 24):
    """The patterns lo, lo + stride, ... < hi in pieces of at most `chunk` elements: (first pattern, count) each."""
    n = (hi - lo + stride - 1) // stride
    return [(lo + i * stride, min(chunk, n - i)) for i in range(0, n, chunk)]


def count_in(a, b, lo, hi, stride):
    """How many of the patterns lo, lo + stride, ... < hi lie in [a, b]."""
    b = min(b, hi - 1)
    if b < a:
        return 0
    first = max(0, -(-(a - lo) // stride))
    last = (b - lo) // stride
    return max(0, last - first + 1)


def in_threads(fn, items, workers=12):
    """fn over items on a few threads (the referees are ctypes calls: they run without the interpreter lock)."""
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(fn, items))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)
