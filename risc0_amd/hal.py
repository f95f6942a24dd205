"""Python mirror of the risc0_zkp `Hal` trait over the r0hip C ABI.

`HipHal` exposes the same method names and argument meanings as
risc0/zkp/src/hal/mod.rs:55-258 (buffers are device allocations of u32 words:
Elem = 1 word, ExtElem = 4, Digest = 8), so the parity tests read like the
reference's DualHal tests (risc0/zkp/src/hal/mod.rs:319-616). It is a thin
ctypes layer: every operation runs in libr0hip.so on the GPU. There is no CPU
fallback; a missing library or device raises.
"""
import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# R0HIP_LIB selects an alternative build of the same library (tools/ experiments only)
LIB_PATH = os.environ.get("R0HIP_LIB") or os.path.join(_HERE, "lib", "libr0hip.so")

POSEIDON2, SHA256, POSEIDON254 = 0, 1, 2
SUITES = {"poseidon2": POSEIDON2, "sha-256": SHA256, "poseidon_254": POSEIDON254, "poseidon254": POSEIDON254}

_lib = None
u32p = C.POINTER(C.c_uint32)


class R0HipError(RuntimeError):
    pass


def lib():
    """Load libr0hip.so (built by __graft_entry__.build()); raise if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise R0HipError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        _declare(L)
        _lib = L
    return _lib


def _declare(L):
    sz = C.c_size_t
    vp = C.c_void_p
    sig = {
        "r0hip_init": [C.c_int],
        "r0hip_device_info": [C.c_char_p, sz, C.POINTER(C.c_uint64)],
        "r0hip_alloc": [C.POINTER(vp), sz],
        "r0hip_free": [vp],
        "r0hip_memset32": [vp, C.c_uint32, sz],
        "r0hip_memcpy_h2d": [vp, vp, sz],
        "r0hip_memcpy_d2h": [vp, vp, sz],
        "r0hip_memcpy_d2d": [vp, vp, sz],
        "r0hip_host_alloc": [C.POINTER(vp), sz],
        "r0hip_host_free": [vp],
        "r0hip_memcpy_d2h_start": [vp, vp, sz, C.POINTER(vp)],
        "r0hip_copy_finish": [vp, C.c_int, C.POINTER(C.c_int)],
        "r0hip_fill_uniform": [vp, sz, C.c_uint64],
        "r0hip_fill_chacha20": [vp, sz, u32p, u32p],
        "r0hip_rv32im_accum_finalize": [vp, sz, sz, sz],
        "r0hip_rv32im_accum": [vp, vp, vp, vp, sz, sz, sz],
        "r0hip_recursion_accum": [vp, vp, vp, vp, vp, sz, sz],
        "r0hip_prove_segments": [C.c_char_p, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p, sz, C.c_uint32],
        "r0hip_prove_trace_segments": [C.c_int, C.c_uint32, C.c_void_p, sz, C.c_uint32, C.c_int],
        "r0hip_verify_seal": [C.c_char_p, C.c_int, u32p, sz, u32p, sz, u32p, C.POINTER(C.c_uint32)],
        "r0hip_testing_verify_seal_structure": [C.c_char_p, C.c_int, u32p, sz, C.POINTER(C.c_uint32)],
        "r0hip_verify_seal_on": [C.c_int, C.c_char_p, C.c_int, u32p, sz, u32p, sz, u32p, C.POINTER(C.c_uint32)],
        "r0hip_testing_verify_seal_structure_on": [C.c_int, C.c_char_p, C.c_int, u32p, sz, C.POINTER(C.c_uint32)],
        "r0hip_merkle_open_digests": [C.c_int, u32p, sz, vp, sz, u32p, u32p],
        "r0hip_set_verify_device_poseidon254": [C.c_int],
        "r0hip_poly_ext": [C.c_char_p, u32p, u32p, u32p, u32p, u32p],
        "r0hip_constraint_rows": [C.c_char_p, C.c_uint32, vp, vp, vp, vp, vp, u32p, vp, vp],
        "r0hip_constraint_term": [C.c_char_p, u32p, u32p, u32p, u32p, C.POINTER(C.c_int32)],
        "r0hip_set_witness_check": [C.c_int, C.POINTER(C.c_int)],
        "r0hip_worker_set_witness_check": [vp, C.c_int],
        "r0hip_synchronize": [],
        "r0hip_set_deferred": [C.c_int, C.POINTER(C.c_int)],
        "r0hip_set_proof_streams": [C.c_uint32, C.POINTER(C.c_uint32)],
        "r0hip_call_stats": [C.POINTER(C.c_uint64)],
        "r0hip_eval_check_launched": [C.POINTER(C.c_int)],
        "r0hip_testing_zero_scan": [vp, sz, sz, C.POINTER(C.c_uint64)],
        "r0hip_batch_expand_into_evaluate_ntt": [vp, vp, sz, C.c_uint32, C.c_uint32],
        "r0hip_batch_interpolate_ntt": [vp, sz, C.c_uint32],
        "r0hip_zk_shift": [vp, sz, C.c_uint32],
        "r0hip_batch_bit_reverse": [vp, sz, C.c_uint32],
        "r0hip_batch_evaluate_any": [vp, vp, sz, C.c_uint32, vp, vp, sz],
        "r0hip_mix_poly_coeffs": [vp, vp, u32p, u32p, u32p, sz, sz],
        "r0hip_fri_fold": [vp, vp, u32p, sz],
        "r0hip_combos_prepare": [vp, u32p, sz, sz, u32p, u32p, sz, u32p],
        "r0hip_poly_divide": [vp, sz, u32p, u32p],
        "r0hip_combos_divide": [vp, sz, u32p, u32p, sz, C.POINTER(C.c_int64)],
        "r0hip_eltwise_add_elem": [vp, vp, vp, sz],
        "r0hip_eltwise_copy_elem": [vp, vp, sz],
        "r0hip_eltwise_zeroize_elem": [vp, sz],
        "r0hip_eltwise_sum_extelem": [vp, vp, sz, sz],
        "r0hip_eltwise_copy_elem_slice": [vp, vp, sz, sz, sz, sz, sz, sz],
        "r0hip_gather_sample": [vp, vp, sz, sz, sz],
        "r0hip_gather_sample_host": [vp, vp, sz, sz, sz],
        "r0hip_merkle_paths_host": [vp, vp, sz, vp, sz, sz],
        "r0hip_scatter": [vp, vp, vp, vp, sz],
        "r0hip_prefix_products": [vp, sz],
        "r0hip_hash_rows": [C.c_int, vp, vp, sz, sz],
        "r0hip_hash_fold": [C.c_int, vp, sz, sz],
        "r0hip_merkle_tree": [C.c_int, vp, vp, sz, sz],
        "r0hip_eval_check": [C.c_char_p, vp, C.POINTER(vp), vp, vp, u32p, C.c_uint32],
        "r0hip_prove_segment": [C.c_char_p, C.c_int, C.c_uint32, vp, vp, vp, vp, C.c_int, C.c_uint32, u32p, sz,
                                C.POINTER(sz), u32p],
        "r0hip_prove_segment_accum": [C.c_char_p, C.c_int, C.c_uint32, vp, vp, vp, sz, vp, sz, vp, C.c_int,
                                      C.c_uint32, u32p, sz, C.POINTER(sz), u32p],
        "r0hip_rv32im_bigint_accum_states": [u32p, vp, sz, sz, u32p],
        "r0hip_rv32im_bigint_accum_states_device": [vp, u32p, vp, sz, sz],
        "r0hip_recursion_witgen": [vp, vp, vp, sz, u32p, sz, u32p, sz, u32p, sz],
        "r0hip_rv32im_witgen": [C.c_uint32, vp, vp, C.c_uint32],
        "r0hip_prove_segment_trace_resident": [C.c_int, C.c_uint32, C.c_uint32, vp, vp, sz, vp, vp, vp, vp, sz,
                                               u32p, sz, C.POINTER(sz), u32p],
        "r0hip_prove_segment_trace": [C.c_int, C.c_uint32, C.c_uint32, u32p, u32p, sz, u32p, u32p, vp, vp, sz, u32p,
                                      sz, C.POINTER(sz), u32p],
        "r0hip_rv32im_inject_backs": [vp, sz, vp, vp],
        "r0hip_prove_segment_trace_backs": [C.c_int, C.c_uint32, C.c_uint32, u32p, vp, vp, u32p, sz, C.POINTER(sz),
                                            u32p],
        "r0hip_prove_recursion": [C.c_int, C.c_uint32, vp, u32p, sz, u32p, sz, u32p, sz, C.c_uint64, u32p, sz,
                                  C.POINTER(sz), u32p],
        "r0hip_prove_recursion_keyed": [C.c_int, C.c_uint32, vp, u32p, sz, u32p, sz, u32p, sz, u32p, C.c_uint64, u32p,
                                        sz, C.POINTER(sz), u32p],
        "r0hip_recursion_program_create": [C.POINTER(vp), C.c_int, C.c_uint32, u32p, sz, C.c_int],
        "r0hip_recursion_program_info": [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(sz), u32p,
                                         C.POINTER(C.c_uint64)],
        "r0hip_recursion_program_ctrl": [vp, C.POINTER(vp)],
        "r0hip_prove_recursion_program": [vp, u32p, sz, u32p, sz, u32p, sz, u32p, C.c_uint64, u32p, sz, C.POINTER(sz),
                                          u32p],
        "r0hip_recursion_program_destroy": [vp],
        "r0hip_recursion_preflight": [u32p, sz, C.c_int, C.c_uint32, u32p, sz, u32p, sz, C.POINTER(sz), u32p, sz,
                                      C.POINTER(sz), u32p, sz, C.POINTER(sz), u32p, sz, C.POINTER(sz)],
        "r0hip_recursion_program_prepare_input": [vp],
        "r0hip_recursion_last_preflight_ms": [C.POINTER(C.c_double)],
        "r0hip_recursion_program_input_info": [vp, vp],
        "r0hip_prove_recursion_program_input": [vp, u32p, sz, u32p, C.c_uint64, u32p, sz, C.POINTER(sz), u32p, u32p,
                                                sz, C.POINTER(sz)],
        "r0hip_worker_create": [C.POINTER(vp), C.c_uint32, C.c_uint32, C.c_int, u32p],
        "r0hip_worker_submit": [vp, vp],
        "r0hip_worker_wait": [vp, C.POINTER(vp), C.c_int64],
        "r0hip_worker_destroy": [vp],
        "r0hip_worker_set_preflight_threads": [vp, C.c_uint32, C.POINTER(C.c_uint32)],
        "r0hip_worker_get_stats": [vp, vp, sz],
        "r0hip_rv32im_bigint_accum_inject": [vp, sz, u32p, vp, sz],
        "r0hip_circuit_info": [C.c_char_p, vp, sz, C.c_char_p, sz],
        "r0hip_circuit_register": [vp, sz],
        "r0hip_circuit_load": [C.c_char_p, C.c_char_p, sz],
        "r0hip_circuit_backend": [C.c_char_p, C.POINTER(C.c_int)],
        "r0hip_testing_set_interp_chunk": [C.c_uint32, u32p],
        "r0hip_prove_segment_cb": [C.c_char_p, C.c_int, C.c_uint32, vp, vp, vp, vp, vp, C.c_int, C.c_uint32, u32p, sz,
                                   C.POINTER(sz), u32p],
        "r0hip_demo_witness": [C.c_uint32, sz, C.c_uint32, C.c_uint32, vp, vp, vp],
        "r0hip_demo_accum": [C.c_uint32, sz, vp, u32p, vp],
        "r0hip_selftest": [C.c_uint32, C.c_uint32, vp, sz],
        "r0hip_last_profile": [C.c_char_p, sz],
        "r0hip_set_kernel_timing": [C.c_int],
        "r0hip_kernel_times": [C.c_char_p, sz],
        "r0hip_mem_stats": [C.POINTER(C.c_uint64)],
        "r0hip_mem_reset_peak": [],
        "r0hip_trim": [],
    }
    for name, args in sig.items():
        if os.environ.get("R0HIP_LIB") and not hasattr(L, name):
            continue  # an older build under R0HIP_LIB (tools/ A/B runs): calling what it lacks raises
        f = getattr(L, name)
        f.argtypes = args
        f.restype = C.c_void_p
    L.r0hip_free_error.argtypes = [C.c_void_p]
    L.r0hip_free_error.restype = None


def check(err):
    if err:
        msg = C.cast(err, C.c_char_p).value.decode()
        lib().r0hip_free_error(err)
        raise R0HipError(msg)


def exported_symbols():
    """Every r0hip_* entry point declared in include/r0hip.h."""
    hdr = os.path.join(os.path.dirname(_HERE), "include", "r0hip.h")
    import re
    return sorted(set(re.findall(r"\b(r0hip_\w+)\s*\(", open(hdr).read())))


def _h(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a, a.ctypes.data_as(u32p)


class Buffer:
    """A device allocation of `size` elements of `words` u32 each (hal/mod.rs:39-53)."""

    def __init__(self, hal, name, size, words=1, ptr=None, owner=True):
        self.hal, self.name, self.size, self.words = hal, name, size, words
        self._owner = owner
        if ptr is None:
            p = C.c_void_p()
            check(lib().r0hip_alloc(C.byref(p), max(1, size * words) * 4))
            ptr = p.value
        self.ptr = ptr

    @property
    def nwords(self):
        return self.size * self.words

    def slice(self, offset, size):
        return Buffer(self.hal, self.name, size, self.words, self.ptr + offset * self.words * 4, owner=False)

    def to_numpy(self):
        out = np.empty(self.nwords, dtype=np.uint32)
        if self.nwords:
            check(lib().r0hip_memcpy_d2h(out.ctypes.data, self.ptr, self.nwords * 4))
        return out

    def copy_from(self, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint32).reshape(-1)
        assert a.size == self.nwords, (a.size, self.nwords)
        if a.size:
            check(lib().r0hip_memcpy_h2d(self.ptr, a.ctypes.data, a.size * 4))

    def free(self):
        if self._owner and self.ptr:
            check(lib().r0hip_free(self.ptr))
        self.ptr = 0

    def __del__(self):
        try:
            if self._owner and self.ptr and _lib is not None:
                _lib.r0hip_free(self.ptr)
        except Exception:
            pass


def _lg(n):
    l = int(n).bit_length() - 1
    assert 1 << l == n, f"{n} is not a power of two"
    return l


class HipHal:
    """risc0_zkp::hal::Hal on MI355X (one instance per process/device)."""

    EXT_SIZE = 4
    CHECK_SIZE = 16

    def __init__(self, hashfn="poseidon2", device=0, deferred=False):
        self.suite = SUITES[hashfn] if isinstance(hashfn, str) else int(hashfn)
        check(lib().r0hip_init(device))
        if deferred:
            self.set_deferred(True)

    # ---- completion mode of the calling thread (r0hip_set_deferred) ----
    def set_deferred(self, on):
        """Device-only calls of this thread return with their work queued (on) or complete
        (off, the default); turning it off drains the thread's stream. Returns the previous
        mode. Reads (to_numpy, combos_divide, eval_check, the prove_* calls) always drain. A
        thread that turned it on turns it off, or synchronises, before it exits."""
        was = C.c_int(0)
        check(lib().r0hip_set_deferred(1 if on else 0, C.byref(was)))
        return bool(was.value)

    @contextlib.contextmanager
    def deferred(self, on=True):
        """`with hal.deferred():` the mode for a block of calls, restored (and drained) after it"""
        was = self.set_deferred(on)
        try:
            yield self
        finally:
            self.set_deferred(was)

    # ---- streams one proof of the calling thread may use (r0hip_set_proof_streams) ----
    def set_proof_streams(self, n):
        return set_proof_streams(n)

    @contextlib.contextmanager
    def proof_streams(self, n):
        """`with hal.proof_streams(2):` the setting for a block of calls, restored after it"""
        was = set_proof_streams(n)
        try:
            yield self
        finally:
            set_proof_streams(was)

    # ---- constraint check of the witness inside the provers (r0hip_set_witness_check) ----
    def set_witness_check(self, on):
        return set_witness_check(on)

    @contextlib.contextmanager
    def witness_check(self, on=True):
        """`with hal.witness_check():` the mode for a block of calls, restored after it"""
        was = set_witness_check(on)
        try:
            yield self
        finally:
            set_witness_check(was)

    def constraint_rows(self, circuit, po2, code, data, accum, mix, glob, poly_mix=None, out=None):
        return constraint_rows(circuit, po2, code, data, accum, mix, glob, poly_mix, out)

    # ---- allocation (hal/mod.rs:67-100) ----
    def alloc_elem(self, name, size):
        return Buffer(self, name, size, 1)

    def alloc_extelem(self, name, size):
        return Buffer(self, name, size, 4)

    def alloc_digest(self, name, size):
        return Buffer(self, name, size, 8)

    def alloc_u32(self, name, size):
        return Buffer(self, name, size, 1)

    def alloc_elem_init(self, name, size, value):
        b = self.alloc_elem(name, size)
        check(lib().r0hip_memset32(b.ptr, value, size))
        return b

    def alloc_extelem_zeroed(self, name, size):
        b = self.alloc_extelem(name, size)
        check(lib().r0hip_memset32(b.ptr, 0, size * 4))
        return b

    def copy_from_elem(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint32).reshape(-1)
        b = self.alloc_elem(name, a.size)
        b.copy_from(a)
        return b

    copy_from_u32 = copy_from_elem

    def copy_from_extelem(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint32).reshape(-1)
        b = self.alloc_extelem(name, a.size // 4)
        b.copy_from(a)
        return b

    def copy_from_digest(self, name, arr):
        a = np.ascontiguousarray(arr, dtype=np.uint32).reshape(-1)
        b = self.alloc_digest(name, a.size // 8)
        b.copy_from(a)
        return b

    def has_unified_memory(self):
        return False

    # ---- HAL ops ----
    def batch_expand_into_evaluate_ntt(self, output, input, count, expand_bits):
        out_size = output.size // count
        check(lib().r0hip_batch_expand_into_evaluate_ntt(output.ptr, input.ptr, count, _lg(out_size), expand_bits))

    def batch_interpolate_ntt(self, io, count):
        check(lib().r0hip_batch_interpolate_ntt(io.ptr, count, _lg(io.size // count)))

    def batch_bit_reverse(self, io, count):
        check(lib().r0hip_batch_bit_reverse(io.ptr, count, _lg(io.size // count)))

    def zk_shift(self, io, count):
        check(lib().r0hip_zk_shift(io.ptr, count, _lg(io.size // count)))

    def batch_evaluate_any(self, coeffs, poly_count, which, xs, out):
        check(lib().r0hip_batch_evaluate_any(out.ptr, coeffs.ptr, poly_count, _lg(coeffs.size // poly_count),
                                             which.ptr, xs.ptr, which.size))

    def mix_poly_coeffs(self, out, mix_start, mix, input, combos, input_size, count):
        cb, cp = _h(combos)
        ms, msp = _h(mix_start)
        mx, mxp = _h(mix)
        check(lib().r0hip_mix_poly_coeffs(out.ptr, input.ptr, cp, msp, mxp, input_size, count))

    def eltwise_add_elem(self, output, input1, input2):
        assert output.size == input1.size == input2.size
        check(lib().r0hip_eltwise_add_elem(output.ptr, input1.ptr, input2.ptr, output.size))

    def eltwise_sum_extelem(self, output, input):
        count = output.size // 4
        check(lib().r0hip_eltwise_sum_extelem(output.ptr, input.ptr, input.size // count, count))

    def eltwise_copy_elem(self, output, input):
        assert output.size == input.size
        check(lib().r0hip_eltwise_copy_elem(output.ptr, input.ptr, output.size))

    def eltwise_copy_elem_slice(self, into, frm, from_rows, from_cols, from_offset, from_stride, into_offset,
                                into_stride):
        src = self.copy_from_elem("from", frm)
        check(lib().r0hip_eltwise_copy_elem_slice(into.ptr, src.ptr, from_rows, from_cols, from_offset, from_stride,
                                                  into_offset, into_stride))

    def eltwise_zeroize_elem(self, elems):
        check(lib().r0hip_eltwise_zeroize_elem(elems.ptr, elems.size))

    def fri_fold(self, output, input, mix):
        m, mp = _h(mix)
        check(lib().r0hip_fri_fold(output.ptr, input.ptr, mp, output.size // 4))

    def hash_rows(self, output, matrix):
        rows = output.size
        check(lib().r0hip_hash_rows(self.suite, output.ptr, matrix.ptr, rows, matrix.size // rows))

    def hash_fold(self, io, input_size, output_size):
        check(lib().r0hip_hash_fold(self.suite, io.ptr, input_size, output_size))

    def merkle_tree(self, nodes, matrix, rows):
        """nodes (2*rows digests) <- leaves and every layer (r0hip_merkle_tree)"""
        check(lib().r0hip_merkle_tree(self.suite, nodes.ptr, matrix.ptr, rows, matrix.size // rows))

    def gather_sample(self, dst, src, idx, size, stride):
        check(lib().r0hip_gather_sample(dst.ptr, src.ptr, idx, size, stride))

    def gather_sample_host(self, src, idx, size, stride):
        """src[idx + i*stride], i < size, as a host array (r0hip_gather_sample_host)"""
        out = np.zeros(size, np.uint32)
        check(lib().r0hip_gather_sample_host(out.ctypes.data, src.ptr, idx, size, stride))
        return out

    def merkle_paths_host(self, nodes, idx, levels):
        """the sibling paths of the openings at node indices idx of a node heap (root at 1), as
        an (n, levels, 8) host array: [i, 0] = nodes[idx[i]], [i, k] = nodes[(idx[i] >> k) ^ 1]
        (r0hip_merkle_paths_host; prove/merkle.rs:131-138)"""
        j = np.ascontiguousarray(idx, dtype=np.uint64).reshape(-1)
        out = np.zeros((j.size, max(int(levels), 0), 8), np.uint32)
        check(lib().r0hip_merkle_paths_host(out.ctypes.data, nodes.ptr, nodes.size, j.ctypes.data, j.size, levels))
        return out

    def scatter(self, into, index, offsets, values):
        index = np.asarray(index, dtype=np.uint32)
        if index.size == 0:
            return
        di, dof, dv = (self.copy_from_u32("index", index), self.copy_from_u32("offsets", offsets),
                       self.copy_from_elem("values", values))
        check(lib().r0hip_scatter(into.ptr, di.ptr, dof.ptr, dv.ptr, index.size - 1))

    def rv32im_accum_finalize(self, accum, rows, cols, last_cycle):
        """accumulation phases 2-3 of risc0_circuit_rv32im_cuda_accum (ffi.cu:480-509)"""
        check(lib().r0hip_rv32im_accum_finalize(accum.ptr, rows, cols, last_cycle))

    def rv32im_accum(self, data, accum, glob, mix, rows, last_cycle):
        """the whole rv32im accumulation, phases 1-3 (risc0_circuit_rv32im_cuda_accum,
        ffi.cu:362-514): `accum` (103 columns of `rows`) starts all-INVALID"""
        check(lib().r0hip_rv32im_accum(data.ptr, accum.ptr, glob.ptr, mix.ptr, rows, 103, last_cycle))

    def recursion_accum(self, ctrl, glob, data, mix, accum, work_cycles, total_cycles):
        """CircuitAccumulator::accumulate of the recursion circuit (witgen.rs:162-170 ->
        risc0_circuit_recursion_cuda_accum): compute, prefix product, verify"""
        check(lib().r0hip_recursion_accum(ctrl.ptr, glob.ptr, data.ptr, mix.ptr, accum.ptr, work_cycles,
                                          total_cycles))

    def prefix_products(self, io):
        check(lib().r0hip_prefix_products(io.ptr, io.size))

    def combos_prepare(self, combos, coeff_u, combo_count, cycles, reg_sizes, reg_combo_ids, mix):
        u, up = _h(coeff_u)
        rs, rsp = _h(reg_sizes)
        rc, rcp = _h(reg_combo_ids)
        m, mp = _h(mix)
        check(lib().r0hip_combos_prepare(combos.ptr, up, combo_count, cycles, rsp, rcp, rs.size, mp))

    def combos_divide(self, combos, chunk_pows, chunk_begin, cycles):
        pw, pwp = _h(chunk_pows)
        bg, bgp = _h(chunk_begin)
        bad = C.c_int64(0)
        check(lib().r0hip_combos_divide(combos.ptr, bg.size - 1, pwp, bgp, cycles, C.byref(bad)))
        return bad.value

    def eval_check(self, circuit, check_buf, groups, mix, glob, poly_mix, po2):
        arr = (C.c_void_p * len(groups))(*[g.ptr for g in groups])
        pm, pmp = _h(poly_mix)
        check(lib().r0hip_eval_check(circuit.encode(), check_buf.ptr, arr, mix.ptr, glob.ptr, pmp, po2))

    def synchronize(self):
        check(lib().r0hip_synchronize())


def prove_segment(hal, circuit, po2, code, data, accum, glob, version=None, seal_cap=1 << 24):
    """Prove one segment from device-resident witness groups; returns (seal, mix)."""
    mix_size = circuit_info(circuit)["mix_size"]  # any circuit compiled in, plugged-in ones included
    seal = np.zeros(seal_cap, dtype=np.uint32)
    n = C.c_size_t(0)
    mix = np.zeros(mix_size, dtype=np.uint32)
    check(lib().r0hip_prove_segment(circuit.encode(), hal.suite, po2, code.ptr, data.ptr, accum.ptr, glob.ptr,
                                    int(version is not None), version or 0, seal.ctypes.data_as(u32p), seal_cap,
                                    C.byref(n), mix.ctypes.data_as(u32p)))
    return seal[: n.value].copy(), mix


class CircuitDesc(C.Structure):
    """struct r0hip_circuit_desc"""
    _fields_ = [("group_sizes", C.c_uint32 * 3), ("mix_size", C.c_uint32), ("output_size", C.c_uint32),
                ("n_taps", C.c_uint32), ("info", C.c_uint8 * 16)]


def circuit_names():
    """r0hip_circuit_info(NULL): the circuits compiled into the library, in build order (the shipped
    ones, "demo", then those plugged in at build time with EXTRA_CIRCUIT_DIRS). Host-only."""
    buf = C.create_string_buffer(4096)
    check(lib().r0hip_circuit_info(None, None, 0, buf, 4096))
    return buf.value.decode().split()


def circuit_info(circuit):
    """r0hip_circuit_info: {"name", "group_sizes" (accum, code, data), "mix_size", "output_size",
    "n_taps", "info" (16 bytes)} of a circuit compiled in. Host-only."""
    d = CircuitDesc()
    check(lib().r0hip_circuit_info(circuit.encode() if circuit is not None else b"", C.byref(d), C.sizeof(d), None, 0))
    return {"name": circuit, "group_sizes": [int(x) for x in d.group_sizes], "mix_size": int(d.mix_size),
            "output_size": int(d.output_size), "n_taps": int(d.n_taps), "info": bytes(d.info)}


class CircuitTables(C.Structure):
    """struct r0hip_circuit_tables"""
    _fields_ = [("name", C.c_char_p), ("taps", u32p), ("n_taps", C.c_size_t), ("combo_taps", u32p),
                ("n_combo_taps", C.c_size_t), ("combo_begin", u32p), ("combos_count", C.c_size_t),
                ("group_begin", u32p), ("n_groups", C.c_size_t), ("group_sizes", u32p), ("poly_mix_powers", u32p),
                ("n_poly_mix", C.c_size_t), ("info", C.c_uint8 * 16), ("mix_size", C.c_size_t),
                ("output_size", C.c_size_t), ("eval_args", C.POINTER(C.c_int32)), ("n_eval_args", C.c_size_t),
                ("ir", u32p), ("n_ir", C.c_size_t)]


def circuit_tables_struct(t, name=None):
    """The r0hip_circuit_tables of a circuit_tables.load() dict, and the arrays it points into
    (keep them alive for as long as the struct is used)."""
    keep = {k: np.ascontiguousarray(t[k], dtype=np.uint32) for k in
            ("taps", "combo_taps", "combo_begin", "group_begin", "group_sizes", "poly_mix_powers", "ir")}
    keep["eval_args"] = np.ascontiguousarray(t["eval_args"], dtype=np.int32)
    s = CircuitTables()
    s.name = (name if name is not None else t["name"]).encode()
    for k, a in keep.items():
        setattr(s, k, a.ctypes.data_as(C.POINTER(C.c_int32) if k == "eval_args" else u32p))
    s.n_taps, s.n_combo_taps, s.combos_count = t["n_taps"], len(t["combo_taps"]), t["combos_count"]
    s.n_groups, s.n_poly_mix, s.n_eval_args, s.n_ir = t["n_groups"], len(t["poly_mix_powers"]), len(t["eval_args"]), t["n_ir"]
    s.mix_size, s.output_size = t["mix_size"], t["output_size"]
    info = t["circuit_info"].encode() if isinstance(t["circuit_info"], str) else bytes(t["circuit_info"])
    if len(info) != 16:
        raise R0HipError(f"circuit_info: {t['circuit_info']!r} is not 16 bytes")
    s.info = (C.c_uint8 * 16)(*info)
    return s, keep


def register_circuit(name, directory, files=None):
    """r0hip_circuit_register: make the circuit of <directory>/<name>.poly.ir and <name>.taps.json
    (the two files a build-time plug-in is; `files` names them when they are not called <name>)
    known to this process under `name`. Every
    circuit-generic call then takes the name; its eval_check and constraint-rows check are
    interpreted on the device, slower than a circuit that was compiled in. The library validates
    the tables and raises with the field named. Host-only."""
    from . import circuit_tables
    base = os.path.join(directory, files if files is not None else name)
    t = circuit_tables.load(base + ".taps.json", base + ".poly.ir")
    s, keep = circuit_tables_struct(t, name)
    check(lib().r0hip_circuit_register(C.byref(s), C.sizeof(s)))


def load_circuit_module(path):
    """r0hip_circuit_load: load the circuit module at `path` (build_circuit_module) into this
    process and return its circuit's name. Every circuit-generic call then takes the name and runs
    the module's generated kernels, as a compiled-in circuit's. The library checks the module's
    ABI number, struct sizes, architecture, tables and kernel view first and raises with the path
    and what disagrees. Loading runs the module's code, exactly as linking it would. Host-only."""
    name = C.create_string_buffer(64)
    check(lib().r0hip_circuit_load(os.fsencode(path), name, 64))
    return name.value.decode()


def circuit_backend(name):
    """r0hip_circuit_backend: 0 compiled in, 1 registered (interpreted on the device), 2 a circuit
    module. Host-only."""
    kind = C.c_int(-1)
    check(lib().r0hip_circuit_backend(name.encode(), C.byref(kind)))
    return int(kind.value)


MODULE_DIR = os.path.join(_HERE, "modules")  # where the default build puts the tests' modules


def build_circuit_module(name, directory, out, jobs=None):
    """Compile the circuit of <directory>/<name>.poly.ir and <name>.taps.json (and
    <name>.ectune.json, if there is one) into the circuit module `out` (`make module` in
    risc0_amd/csrc: the generators, then hipcc for the library's architecture). Returns out."""
    import subprocess
    jobs = jobs or min(16, os.cpu_count() or 8)
    subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-j", str(jobs), "module", f"NAME={name}",
                           f"DIR={os.path.abspath(directory)}", f"OUT={os.path.abspath(out)}"])
    return out


def testing_set_interp_chunk(points):
    """r0hip_testing_set_interp_chunk (TESTING ONLY): the points per interpreter launch on this
    thread, 0 = the slot-file budget's choice; returns the previous value."""
    was = C.c_uint32(0)
    check(lib().r0hip_testing_set_interp_chunk(points, C.byref(was)))
    return int(was.value)


ACCUM_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, u32p, C.c_void_p, C.c_void_p)  # r0hip_accum_fn


def prove_segment_cb(hal, circuit, po2, code, data, accum_fn, glob, version=None, seal_cap=1 << 24):
    """r0hip_prove_segment_cb: prove_segment with the accum group made after the mix is drawn.
    accum_fn(mix, accum, stream) is called on this thread with the mix (numpy, mix_size words), the
    library's accum group as a Buffer (2^po2 x group_sizes[0] words, INVALID-filled; valid only
    during the call) and the stream; it fills the group (copy_from, demo_accum, any per-op call) and
    returns None, or a str that fails the proof. Returns (seal, mix)."""
    info = circuit_info(circuit)
    rows, cols, mix_size = 1 << po2, info["group_sizes"][0], info["mix_size"]
    keep = []  # the message's bytes must outlive the callback's return

    def tramp(_user, h_mix, d_accum, stream):
        try:
            mix = np.ctypeslib.as_array(h_mix, shape=(mix_size,)).copy() if mix_size else np.zeros(0, np.uint32)
            msg = accum_fn(mix, Buffer(hal, "accum", rows * cols, 1, ptr=d_accum, owner=False), stream)
        except Exception as e:  # never unwind through the C frames
            msg = f"{type(e).__name__}: {e}"
        if msg is None:
            return None
        keep.append(C.create_string_buffer(str(msg).encode()))
        return C.addressof(keep[-1])

    fn = ACCUM_FN(tramp)
    seal = np.zeros(seal_cap, dtype=np.uint32)
    n = C.c_size_t(0)
    mix = np.zeros(mix_size, dtype=np.uint32)
    check(lib().r0hip_prove_segment_cb(circuit.encode(), hal.suite, po2, code.ptr, data.ptr, C.cast(fn, C.c_void_p), None,
                                       glob.ptr, int(version is not None), version or 0, seal.ctypes.data_as(u32p),
                                       seal_cap, C.byref(n), mix.ctypes.data_as(u32p)))
    return seal[: n.value].copy(), mix


def demo_witness(po2, n_active, a0, b0, code, data, glob):
    """r0hip_demo_witness: the demo circuit's code group (every row), the rows below n_active of its
    data group and its 3 global words, into device Buffers; a0, b0 are Montgomery words."""
    check(lib().r0hip_demo_witness(po2, n_active, a0, b0, code.ptr, data.ptr, glob.ptr))


def demo_accum(po2, n_active, data, mix, accum):
    """r0hip_demo_accum: the rows below n_active of the demo circuit's accum group from its data
    group and the 4 mix words (host)."""
    m, mp = _h(mix)
    assert m.size == 4
    check(lib().r0hip_demo_accum(po2, n_active, data.ptr, mp, accum.ptr))


class SelftestSuite(C.Structure):
    """struct r0hip_selftest_suite"""
    _fields_ = [("passed", C.c_uint32), ("seal_len", C.c_uint32), ("ms", C.c_double * 3)]


class SelftestReport(C.Structure):
    """struct r0hip_selftest_report"""
    _fields_ = [("suite", SelftestSuite * 3)]


def selftest(suites_mask=0b111, po2=10, out_size=None):
    """r0hip_selftest: prove and verify the demo circuit on this card, per hash suite of the mask
    (bit 0 poseidon2, 1 sha-256, 2 poseidon254). Returns (error or None, {suite id: {"passed":
    bits a|b<<1|c<<2, "seal_len", "ms": [a, b, c]}}); error is None only when every check asked
    for passed. Refusals of the arguments raise R0HipError."""
    rep = SelftestReport()
    err = lib().r0hip_selftest(suites_mask, po2, C.byref(rep), C.sizeof(rep) if out_size is None else out_size)
    msg = None
    if err:
        msg = C.cast(err, C.c_char_p).value.decode()
        lib().r0hip_free_error(err)
        if not any(s.passed or s.seal_len for s in rep.suite):
            raise R0HipError(msg)
    return msg, {i: {"passed": int(s.passed), "seal_len": int(s.seal_len), "ms": [float(x) for x in s.ms]}
                 for i, s in enumerate(rep.suite) if (suites_mask >> i) & 1}


class BigIntBack(C.Structure):
    """struct r0hip_bigint_back (include/r0hip.h): one Back::BigInt record of the rv32im
    preflight trace (witgen/preflight.rs:55-56; BigIntState, witgen/bigint.rs:36-44)"""
    _fields_ = [("row", C.c_uint32), ("poly_op", C.c_uint32), ("coeff", C.c_uint32), ("bytes", C.c_uint8 * 16)]


#: struct r0hip_bigint_back as a NumPy structured dtype (itemsize 28)
BIGINT_BACK_DTYPE = np.dtype([("row", "<u4"), ("poly_op", "<u4"), ("coeff", "<u4"), ("bytes", "u1", (16,))])
assert BIGINT_BACK_DTYPE.itemsize == C.sizeof(BigIntBack)


def bigint_backs(records):
    """ctypes array of BigIntBack from [(row, poly_op, coeff, bytes16), ...] or from a
    structured array of BIGINT_BACK_DTYPE, copied whole (None/empty -> None)"""
    if records is None or len(records) == 0:
        return None
    arr = (BigIntBack * len(records))()
    if isinstance(records, np.ndarray):
        assert records.dtype == BIGINT_BACK_DTYPE and records.ndim == 1, records.dtype
        rec = np.ascontiguousarray(records)
        C.memmove(arr, rec.ctypes.data, rec.nbytes)
        return arr
    for a, (row, op, coeff, by) in zip(arr, records):
        a.row, a.poly_op, a.coeff = int(row), int(op), int(coeff)
        for i, b in enumerate(by):
            a.bytes[i] = int(b)
    return arr


def bigint_accum_states(mix, records, rows):
    """r0hip_rv32im_bigint_accum_states (host-only): BigIntAccum::step over the records with the
    final mix (byte_poly.rs:381-470); returns (len(records), 12) Montgomery words"""
    arr = bigint_backs(records)
    n = 0 if arr is None else len(arr)
    m, mp = _h(mix)
    out = np.zeros(max(1, n * 12), np.uint32)
    check(lib().r0hip_rv32im_bigint_accum_states(mp, None if arr is None else C.cast(arr, C.c_void_p), n, rows,
                                                 out.ctypes.data_as(u32p)))
    return out[: n * 12].reshape(n, 12)


def bigint_accum_states_device(hal, mix, records, rows):
    """r0hip_rv32im_bigint_accum_states_device: the same states from the device's parallel scans
    (always the device path); returns (len(records), 12) Montgomery words"""
    arr = bigint_backs(records)
    n = 0 if arr is None else len(arr)
    m, mp = _h(mix)
    out = hal.alloc_u32("bigint_states", n * 12)
    check(lib().r0hip_rv32im_bigint_accum_states_device(out.ptr, mp, None if arr is None else C.cast(arr, C.c_void_p),
                                                        n, rows))
    st = out.to_numpy().reshape(n, 12)
    out.free()
    return st


def bigint_accum_inject(accum, rows, mix, records):
    """r0hip_rv32im_bigint_accum_inject: the states scattered into accum columns 0..11"""
    arr = bigint_backs(records)
    m, mp = _h(mix)
    check(lib().r0hip_rv32im_bigint_accum_inject(accum.ptr, rows, mp, None if arr is None else C.cast(arr, C.c_void_p),
                                                 0 if arr is None else len(arr)))


def prove_segment_accum(hal, circuit, po2, code, data, accum, work_cycles, glob, version=None, seal_cap=1 << 24,
                        bigint=None):
    """Prove one segment with the circuit's accumulation on the device between the mix draw and
    the accum commit (r0hip_prove_segment_accum): `accum` holds the group as the witness
    generator allocated it (INVALID words) and is filled in place; `bigint` (rv32im) is the
    trace's BigInt backs [(row, poly_op, coeff, bytes16)], injected with the drawn mix.
    Returns (seal, mix)."""
    backs = bigint_backs(bigint)
    mix_size = circuit_info(circuit)["mix_size"]  # any circuit the library knows, registered ones included
    seal = np.zeros(seal_cap, dtype=np.uint32)
    n = C.c_size_t(0)
    mix = np.zeros(mix_size, dtype=np.uint32)
    check(lib().r0hip_prove_segment_accum(circuit.encode(), hal.suite, po2, code.ptr, data.ptr, accum.ptr,
                                          work_cycles, None if backs is None else C.cast(backs, C.c_void_p),
                                          0 if backs is None else len(backs), glob.ptr, int(version is not None),
                                          version or 0,
                                          seal.ctypes.data_as(u32p), seal_cap, C.byref(n),
                                          mix.ctypes.data_as(u32p)))
    return seal[: n.value].copy(), mix


def _trace(wom, cycles, iops):
    w = np.ascontiguousarray(np.asarray(wom, dtype=np.uint32).reshape(-1))
    c = np.ascontiguousarray(np.asarray(cycles, dtype=np.uint32).reshape(-1))
    i = np.ascontiguousarray(np.asarray(iops, dtype=np.uint32).reshape(-1))
    assert w.size % 4 == 0 and c.size % 2 == 0 and i.size % 4 == 0
    return w, c, i


def recursion_witgen(ctrl, data, glob, total_cycles, wom, cycles, iops):
    """r0hip_recursion_witgen: the recursion circuit's witness generation on the device from
    the control group and the preflight trace (wom: (k, 4) words, cycles: [(iop_idx,
    is_par_safe)], iops: (m, 4) words); data and glob must arrive INVALID-filled."""
    w, c, i = _trace(wom, cycles, iops)
    check(lib().r0hip_recursion_witgen(ctrl.ptr, data.ptr, glob.ptr, total_cycles, w.ctypes.data_as(u32p), w.size // 4,
                                       c.ctypes.data_as(u32p), c.size // 2, i.ctypes.data_as(u32p), i.size // 4))


def prove_recursion(hal, po2, ctrl, wom, cycles, iops, noise_seed, seal_cap=1 << 24):
    """r0hip_prove_recursion: a whole recursion proof from the program's control group and its
    preflight trace (witness generation, ZK noise from noise_seed, accumulation, prove).
    Returns (seal, mix)."""
    w, c, i = _trace(wom, cycles, iops)
    seal = np.zeros(seal_cap, dtype=np.uint32)
    n = C.c_size_t(0)
    mix = np.zeros(20, dtype=np.uint32)
    check(lib().r0hip_prove_recursion(hal.suite, po2, ctrl.ptr, w.ctypes.data_as(u32p), w.size // 4,
                                      c.ctypes.data_as(u32p), c.size // 2, i.ctypes.data_as(u32p), i.size // 4,
                                      noise_seed, seal.ctypes.data_as(u32p), seal_cap, C.byref(n),
                                      mix.ctypes.data_as(u32p)))
    return seal[: n.value].copy(), mix


def _key_words(key):
    """a ChaCha20 key as 8 little-endian words, from 32 bytes or 8 words (None -> NULL: an OS key)"""
    if key is None:
        return None, None
    k = np.frombuffer(bytes(key), dtype="<u4") if isinstance(key, (bytes, bytearray)) else \
        np.ascontiguousarray(key, dtype=np.uint32).reshape(-1)
    if k.size != 8:
        raise R0HipError("a ChaCha20 key is 8 words (32 bytes)")
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return k, k.ctypes.data_as(u32p)


def fill_chacha20(buf, key, nonce, count=None, offset=0):
    """r0hip_fill_chacha20: words [offset, offset + count) of `buf` <- elements 0..count-1 of the
    ChaCha20 stream under key (8 words or 32 bytes) and nonce (3 words): element i is keystream
    words 4i..4i+3 (RFC 8439 section 2.3, block counter from 0) as a 128-bit little-endian
    integer mod p."""
    k, kp = _key_words(key)
    if k is None:
        raise R0HipError("fill_chacha20 needs a key")
    nz, nzp = _h(nonce)
    if nz.size != 3:
        raise R0HipError("a ChaCha20 nonce is 3 words")
    count = buf.nwords - offset if count is None else count
    if offset < 0 or count < 0 or offset + count > buf.nwords:
        raise R0HipError("fill_chacha20: range outside the buffer")
    check(lib().r0hip_fill_chacha20(buf.ptr + 4 * offset, count, kp, nzp))


def prove_recursion_keyed(hal, po2, ctrl, wom, cycles, iops, key, stream_id, seal_cap=1 << 24):
    """r0hip_prove_recursion_keyed: prove_recursion with the ZK noise drawn from the ChaCha20
    stream of `key` (8 words or 32 bytes; None: 32 bytes of getrandom(2) for this call) and
    stream_id (a key must never meet the same stream_id twice). Returns (seal, mix)."""
    w, c, i = _trace(wom, cycles, iops)
    k, kp = _key_words(key)
    seal = np.zeros(seal_cap, dtype=np.uint32)
    n = C.c_size_t(0)
    mix = np.zeros(20, dtype=np.uint32)
    check(lib().r0hip_prove_recursion_keyed(hal.suite, po2, ctrl.ptr, w.ctypes.data_as(u32p), w.size // 4,
                                            c.ctypes.data_as(u32p), c.size // 2, i.ctypes.data_as(u32p), i.size // 4,
                                            kp, stream_id, seal.ctypes.data_as(u32p), seal_cap, C.byref(n),
                                            mix.ctypes.data_as(u32p)))
    return seal[: n.value].copy(), mix


CODE_ENCODED, CODE_MONTGOMERY = 0, 1


class RecursionInputInfo(C.Structure):
    """struct r0hip_recursion_input_info (include/r0hip.h)"""
    _fields_ = [("prepared", C.c_uint32), ("n_runs", C.c_uint32), ("bucket_runs", C.c_uint32 * 9),
                ("n_wom", C.c_size_t), ("n_iops", C.c_size_t), ("n_output", C.c_size_t), ("n_input", C.c_uint64),
                ("plan_device_bytes", C.c_uint64), ("plan_host_bytes", C.c_uint64)]


def recursion_last_preflight_ms():
    """host milliseconds of the preflight inside this thread's last RecursionProgram.prove_input"""
    ms = C.c_double(0)
    check(lib().r0hip_recursion_last_preflight_ms(C.byref(ms)))
    return ms.value


def recursion_preflight(code, po2, inp=(), form=0):
    """r0hip_recursion_preflight: the native preflight of a program's words (row-major, 23 per
    row) on `inp`, host only. Returns (wom (k, 4), cycles (rows, 2), iops (m, 4), output), the
    WOM and IOP values as Montgomery words; raises R0HipError with the preflight's message."""
    c = np.ascontiguousarray(code, dtype=np.uint32).reshape(-1)
    x = np.ascontiguousarray(inp, dtype=np.uint32).reshape(-1)
    n = [C.c_size_t(0) for _ in range(4)]
    xp = x.ctypes.data_as(u32p) if x.size else None
    check(lib().r0hip_recursion_preflight(c.ctypes.data_as(u32p), c.size, form, po2, xp, x.size, None, 0,
                                          C.byref(n[0]), None, 0, C.byref(n[1]), None, 0, C.byref(n[2]), None, 0,
                                          C.byref(n[3])))
    # a word past each count, so that no array is empty (an empty array has no address to give)
    wom, cyc, iops, out = (np.zeros(k.value * w + 1, dtype=np.uint32) for k, w in zip(n, (4, 2, 4, 1)))
    check(lib().r0hip_recursion_preflight(c.ctypes.data_as(u32p), c.size, form, po2, xp, x.size,
                                          wom.ctypes.data_as(u32p), n[0].value, None, cyc.ctypes.data_as(u32p),
                                          n[1].value, None, iops.ctypes.data_as(u32p), n[2].value, None,
                                          out.ctypes.data_as(u32p), n[3].value, None))
    return wom[:-1].reshape(-1, 4), cyc[:-1].reshape(-1, 2), iops[:-1].reshape(-1, 4), out[:-1]


class RecursionProgram:
    """A recursion program resident on the device (r0hip_recursion_program_*): the control group
    and its commitment, made once from the program's rows and reused by every proof.

        with RecursionProgram.create(hal, po2, program.encoded()) as prog:
            suite, po2, rows, control_id, device_bytes = prog.info()
            seal, mix = prog.prove(wom, cycles, iops, key, stream_id)

    `code` is row-major, 23 words per row: plain integers as a .zkr holds them (CODE_ENCODED,
    each word goes through Elem::from) or Program.code's Montgomery words (CODE_MONTGOMERY).
    close() is refused while a proof or a queued worker job still uses the handle."""

    def __init__(self, handle, suite):
        self._h, self.suite = handle, suite

    @classmethod
    def create(cls, hal, po2, code, form=CODE_ENCODED, suite=None, n_words=None):
        """n_words: the program's length when `code` is a longer array (default: all of it)"""
        suite = hal.suite if suite is None else (SUITES[suite] if isinstance(suite, str) else int(suite))
        c = np.ascontiguousarray(code, dtype=np.uint32).reshape(-1)
        if n_words is not None and n_words > c.size:
            raise R0HipError(f"n_words {n_words} is more than the {c.size} words given")
        h = C.c_void_p()
        check(lib().r0hip_recursion_program_create(C.byref(h), suite, po2, c.ctypes.data_as(u32p),
                                                   c.size if n_words is None else n_words, form))
        return cls(h, suite)

    def preflight(self, inp=()):
        """the native preflight of this program on `inp` (recursion_preflight), from the control
        group read back from the device (the handle keeps no host copy of the code)"""
        _suite, po2, rows, _cid, _dev = self.info()
        code = np.ascontiguousarray(self.ctrl().reshape(23, 1 << po2)[:, :rows].T)
        return recursion_preflight(code, po2, inp, CODE_MONTGOMERY)

    def prepare_input(self):
        """r0hip_recursion_program_prepare_input: the op table and the witness generator's plan,
        made once (prove_input and Worker.submit_recursion_input call it themselves)"""
        check(lib().r0hip_recursion_program_prepare_input(self._handle()))

    def input_info(self):
        """r0hip_recursion_program_input_info as a RecursionInputInfo"""
        info = RecursionInputInfo()
        check(lib().r0hip_recursion_program_input_info(self._handle(), C.addressof(info)))
        return info

    def prove_input(self, inp, key, stream_id, seal_cap=1 << 24):
        """r0hip_prove_recursion_program_input: RecursionProver::prove(program, input). Returns
        (seal, mix, output): the seal and mix of prove() on the preflight's arrays with the same
        key and stream_id, and Preflight.output."""
        x = np.ascontiguousarray(inp, dtype=np.uint32).reshape(-1)
        k, kp = _key_words(key)
        seal = np.zeros(seal_cap, dtype=np.uint32)
        n, n_out = C.c_size_t(0), C.c_size_t(0)
        mix = np.zeros(20, dtype=np.uint32)
        h = self._handle()
        info = self.input_info()
        if not info.prepared:  # once: the call below would do it too, but n_output sizes the buffer
            self.prepare_input()
            info = self.input_info()
        out = np.zeros(info.n_output + 1, dtype=np.uint32)
        check(lib().r0hip_prove_recursion_program_input(h, x.ctypes.data_as(u32p) if x.size else None, x.size, kp,
                                                        stream_id, seal.ctypes.data_as(u32p), seal_cap, C.byref(n),
                                                        mix.ctypes.data_as(u32p), out.ctypes.data_as(u32p),
                                                        out.size - 1, C.byref(n_out)))
        return seal[: n.value].copy(), mix, out[: n_out.value].copy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _handle(self):
        if self._h is None or not self._h.value:
            raise R0HipError("the recursion program is closed")
        return self._h

    def info(self):
        """(suite, po2, code_rows, control_id as 8 words, device_bytes)"""
        suite, po2, rows, dev = C.c_int(), C.c_uint32(), C.c_size_t(), C.c_uint64()
        cid = np.zeros(8, dtype=np.uint32)
        check(lib().r0hip_recursion_program_info(self._handle(), C.byref(suite), C.byref(po2), C.byref(rows),
                                                 cid.ctypes.data_as(u32p), C.byref(dev)))
        return suite.value, po2.value, rows.value, cid, dev.value

    def ctrl_ptr(self):
        """device address of the control group (read-only; valid until close)"""
        p = C.c_void_p()
        check(lib().r0hip_recursion_program_ctrl(self._handle(), C.byref(p)))
        return p.value

    def ctrl(self):
        """the control group read back: 23 x 2^po2 Montgomery words, column-major"""
        _suite, po2, _rows, _cid, _dev = self.info()
        out = np.zeros(23 << po2, dtype=np.uint32)
        check(lib().r0hip_memcpy_d2h(out.ctypes.data, self.ctrl_ptr(), out.nbytes))
        return out

    def prove(self, wom, cycles, iops, key, stream_id, seal_cap=1 << 24):
        """r0hip_prove_recursion_program: the seal and mix of prove_recursion_keyed on this
        program's control group with the same key and stream_id"""
        w, c, i = _trace(wom, cycles, iops)
        k, kp = _key_words(key)
        seal = np.zeros(seal_cap, dtype=np.uint32)
        n = C.c_size_t(0)
        mix = np.zeros(20, dtype=np.uint32)
        check(lib().r0hip_prove_recursion_program(self._handle(), w.ctypes.data_as(u32p), w.size // 4,
                                                  c.ctypes.data_as(u32p), c.size // 2, i.ctypes.data_as(u32p),
                                                  i.size // 4, kp, stream_id, seal.ctypes.data_as(u32p), seal_cap,
                                                  C.byref(n), mix.ctypes.data_as(u32p)))
        return seal[: n.value].copy(), mix

    def close(self):
        """r0hip_recursion_program_destroy; raises (and keeps the handle) while it is in use"""
        h = getattr(self, "_h", None)
        if h is None or not h.value:
            return
        check(lib().r0hip_recursion_program_destroy(h))
        self._h = None


class RawBuffer(C.Structure):
    """struct r0hip_raw_buffer (RawBuffer, rv32im-sys/src/lib.rs:63-69)"""
    _fields_ = [("buf", C.c_void_p), ("rows", C.c_size_t), ("cols", C.c_size_t), ("checked", C.c_bool)]


class RawExecBuffers(C.Structure):
    """struct r0hip_raw_exec_buffers (RawExecBuffers, lib.rs:71-75)"""
    _fields_ = [("glob", RawBuffer), ("data", RawBuffer)]


class RawPreflightTrace(C.Structure):
    """struct r0hip_raw_preflight_trace (RawPreflightTrace, lib.rs:53-61): host pointers"""
    _fields_ = [("cycles", C.c_void_p), ("txns", C.c_void_p), ("bigint_bytes", C.c_void_p), ("txns_len", C.c_uint32),
                ("bigint_bytes_len", C.c_uint32), ("table_split_cycle", C.c_uint32)]


def rv32im_witgen(data, glob, cycles, txns, table_split, bigint=None, mode=0):
    """r0hip_rv32im_witgen: the rv32im witness generation (step_Top per cycle, two phases) on
    the device. data (211 x rows) and glob (90 words) are device buffers as the witness
    generator prepares them (INVALID with the injector scattered in); cycles / txns are the
    preflight's RawPreflightCycle / RawMemoryTransaction arrays (numpy structured or raw bytes,
    one record per row)."""
    cyc = np.ascontiguousarray(cycles)
    tx = np.ascontiguousarray(txns)
    bi = np.ascontiguousarray(bigint if bigint is not None else np.zeros(0, np.uint8), dtype=np.uint8)
    rows = data.size // 211
    assert cyc.nbytes == 36 * rows and tx.nbytes % 20 == 0
    bufs = RawExecBuffers(RawBuffer(glob.ptr, 1, glob.size, True), RawBuffer(data.ptr, rows, 211, True))
    pf = RawPreflightTrace(cyc.ctypes.data, tx.ctypes.data if tx.nbytes else None, bi.ctypes.data if bi.size else None,
                           tx.nbytes // 20, bi.size, table_split)
    check(lib().r0hip_rv32im_witgen(mode, C.byref(bufs), C.byref(pf), rows))


def prove_segment_trace(hal, po2, glob, inj_index, inj_offsets, inj_values, cycles, txns, table_split, bigint=None,
                        bigint_records=None, mode=0, seal_cap=1 << 24):
    """r0hip_prove_segment_trace: rv32im prove_core from a preflight trace on the device
    (injector scatter, stepExec, zeroize, accumulation, prove). glob: build_global_vec's 90
    Montgomery words (INVALID where unset); the injector as index / offsets / Montgomery
    values. Returns (seal, mix)."""
    u = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    g, ix, off, val = u(glob), u(inj_index), u(inj_offsets), u(inj_values)
    cyc, tx = np.ascontiguousarray(cycles), np.ascontiguousarray(txns)
    bi = np.ascontiguousarray(bigint if bigint is not None else np.zeros(0, np.uint8), dtype=np.uint8)
    pf = RawPreflightTrace(cyc.ctypes.data, tx.ctypes.data if tx.nbytes else None, bi.ctypes.data if bi.size else None,
                           tx.nbytes // 20, bi.size, table_split)
    backs = bigint_backs(bigint_records)
    nb = 0 if backs is None else len(backs)
    backs = None if backs is None else C.cast(backs, C.c_void_p)
    seal = np.zeros(seal_cap, dtype=np.uint32)
    n = C.c_size_t(0)
    mix = np.zeros(36, dtype=np.uint32)
    check(lib().r0hip_prove_segment_trace(hal.suite, po2, mode, g.ctypes.data_as(u32p), ix.ctypes.data_as(u32p),
                                          ix.size - 1, off.ctypes.data_as(u32p), val.ctypes.data_as(u32p), C.byref(pf),
                                          backs, nb, seal.ctypes.data_as(u32p), seal_cap, C.byref(n),
                                          mix.ctypes.data_as(u32p)))
    return seal[: n.value].copy(), mix


class Back(C.Structure):
    """struct r0hip_back (include/r0hip.h): one row's Back record (witgen/preflight.rs:47-57);
    `word` is the index of its payload's first word"""
    _fields_ = [("row", C.c_uint32), ("kind", C.c_uint32), ("word", C.c_uint32)]


class BacksStruct(C.Structure):
    """struct r0hip_backs (include/r0hip.h): the injector as the preflight's Back records"""
    _fields_ = [("recs", C.c_void_p), ("n", C.c_size_t), ("words", C.c_void_p), ("n_words", C.c_size_t),
                ("inj_rows", C.c_size_t)]


BACK_ECALL, BACK_POSEIDON2, BACK_SHA2, BACK_BIGINT = 1, 2, 3, 4
#: payload words of each record kind (R0HIP_BACK_*)
BACK_WORDS = {BACK_ECALL: 3, BACK_POSEIDON2: 39, BACK_SHA2: 10, BACK_BIGINT: 22}


class Backs:
    """r0hip_backs over numpy arrays, kept alive with it: recs is (n, 3) uint32 rows of (row, kind,
    word), words the payloads as plain u32, inj_rows the rows that get the set_cycle columns. The
    arrays are kept as given when they are contiguous uint32 (page-locked views copy at full
    rate); n / n_words default to the arrays' sizes."""

    def __init__(self, recs, words, inj_rows, n=None, n_words=None):
        u = lambda a: a if isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.flags.c_contiguous \
            else np.ascontiguousarray(a, dtype=np.uint32)
        self.recs, self.words, self.inj_rows = u(recs).reshape(-1, 3), u(words).reshape(-1), int(inj_rows)
        self.struct = BacksStruct(self.recs.ctypes.data if self.recs.size else None,
                                  self.recs.shape[0] if n is None else n,
                                  self.words.ctypes.data if self.words.size else None,
                                  self.words.size if n_words is None else n_words, self.inj_rows)

    def nbytes(self):
        return self.recs.nbytes + self.words.nbytes


def rv32im_inject_backs(data, rows, cycles, backs):
    """r0hip_rv32im_inject_backs: build_injector plus hal.scatter from the Back records. data is
    the data group (211 x rows) on the device, cycles the preflight's RawPreflightCycle array
    (at least backs.inj_rows records), backs a Backs."""
    cyc = np.ascontiguousarray(cycles)
    assert backs.inj_rows > rows or cyc.nbytes >= 36 * backs.inj_rows  # inj_rows > rows is refused unread
    check(lib().r0hip_rv32im_inject_backs(data.ptr, rows, cyc.ctypes.data if cyc.nbytes else None,
                                          C.byref(backs.struct)))


def prove_segment_trace_backs(hal, po2, glob, backs, cycles, txns, table_split, bigint=None, mode=0,
                              seal_cap=1 << 24):
    """r0hip_prove_segment_trace_backs: prove_segment_trace with the injector as a Backs (the
    expansion runs on the device, and the accumulation's BigInt records come from the payloads).
    Returns (seal, mix)."""
    g = np.ascontiguousarray(glob, dtype=np.uint32)
    cyc, tx = np.ascontiguousarray(cycles), np.ascontiguousarray(txns)
    bi = np.ascontiguousarray(bigint if bigint is not None else np.zeros(0, np.uint8), dtype=np.uint8)
    pf = RawPreflightTrace(cyc.ctypes.data, tx.ctypes.data if tx.nbytes else None, bi.ctypes.data if bi.size else None,
                           tx.nbytes // 20, bi.size, table_split)
    seal = np.zeros(seal_cap, dtype=np.uint32)
    n = C.c_size_t(0)
    mix = np.zeros(36, dtype=np.uint32)
    check(lib().r0hip_prove_segment_trace_backs(hal.suite, po2, mode, g.ctypes.data_as(u32p), C.byref(pf),
                                                None if backs is None else C.byref(backs.struct),
                                                seal.ctypes.data_as(u32p), seal_cap, C.byref(n),
                                                mix.ctypes.data_as(u32p)))
    return seal[: n.value].copy(), mix


class ResidentTrace:
    """a preflight trace, its injector and global vector uploaded once to device memory, for
    r0hip_prove_segment_trace_resident (the benchmark's inputs-in-HBM form of
    prove_segment_trace)"""

    def __init__(self, hal, po2, glob, inj_index, inj_offsets, inj_values, cycles, txns, table_split, bigint=None):
        u = lambda a: np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)
        self.po2 = po2
        self.glob = hal.copy_from_elem("global", u(glob))
        self.index = hal.copy_from_elem("inj_index", u(inj_index))
        self.inj_rows = self.index.size - 1
        n_inj = max(1, int(np.asarray(inj_index)[-1]))
        self.offsets = hal.copy_from_elem("inj_offsets", u(inj_offsets) if len(inj_offsets) else np.zeros(n_inj, np.uint32))
        self.values = hal.copy_from_elem("inj_values", u(inj_values) if len(inj_values) else np.zeros(n_inj, np.uint32))
        cyc = np.ascontiguousarray(cycles).view(np.uint32).reshape(-1)
        tx = np.ascontiguousarray(txns).view(np.uint32).reshape(-1)
        self.cycles = hal.copy_from_elem("cycles", cyc)
        self.txns = hal.copy_from_elem("txns", tx if tx.size else np.zeros(5, np.uint32))
        bi = np.ascontiguousarray(bigint if bigint is not None else np.zeros(4, np.uint8), dtype=np.uint8)
        pad = (-bi.size) % 4
        self.bigint = hal.copy_from_elem("bigint", np.concatenate([bi, np.zeros(pad, np.uint8)]).view(np.uint32))
        self.pf = RawPreflightTrace(self.cycles.ptr, self.txns.ptr if tx.size else None,
                                    self.bigint.ptr if bigint is not None and len(bigint) else None, tx.size // 5,
                                    0 if bigint is None else len(bigint), table_split)


def prove_segment_trace_resident(hal, t, mode=0, bigint_records=None, seal_cap=1 << 24):
    """r0hip_prove_segment_trace_resident over a ResidentTrace; returns (seal, mix)"""
    backs = bigint_backs(bigint_records)
    nb = 0 if backs is None else len(backs)
    backs = None if backs is None else C.cast(backs, C.c_void_p)
    seal = np.zeros(seal_cap, dtype=np.uint32)
    n = C.c_size_t(0)
    mix = np.zeros(36, dtype=np.uint32)
    check(lib().r0hip_prove_segment_trace_resident(hal.suite, t.po2, mode, t.glob.ptr, t.index.ptr, t.inj_rows,
                                                   t.offsets.ptr, t.values.ptr, C.byref(t.pf), backs, nb,
                                                   seal.ctypes.data_as(u32p), seal_cap, C.byref(n),
                                                   mix.ctypes.data_as(u32p)))
    return seal[: n.value].copy(), mix


class TraceInput(C.Structure):
    """struct r0hip_trace_input (include/r0hip.h): one preflight trace, host pointers"""
    _fields_ = [("mode", C.c_uint32), ("h_global", C.c_void_p), ("h_inj_index", C.c_void_p), ("inj_rows", C.c_size_t),
                ("h_inj_offsets", C.c_void_p), ("h_inj_values", C.c_void_p), ("preflight", RawPreflightTrace)]


class SegmentJob(C.Structure):
    """struct r0hip_segment_job (include/r0hip.h)"""
    _fields_ = [("h_code", C.c_void_p), ("h_data", C.c_void_p), ("h_accum", C.c_void_p), ("h_global", C.c_void_p),
                ("h_bigint", C.c_void_p), ("n_bigint", C.c_size_t), ("h_seal", C.c_void_p),
                ("seal_cap", C.c_size_t), ("seal_len", C.c_size_t), ("h_mix_out", C.c_void_p), ("error", C.c_void_p)]


class TraceJobStruct(C.Structure):
    """struct r0hip_trace_job (include/r0hip.h)"""
    _fields_ = [("trace", TraceInput), ("h_bigint", C.c_void_p), ("n_bigint", C.c_size_t), ("h_seal", C.c_void_p),
                ("seal_cap", C.c_size_t), ("seal_len", C.c_size_t), ("h_mix_out", C.c_void_p), ("error", C.c_void_p),
                ("verified", C.c_int), ("verify_ms", C.c_double), ("prove_ms", C.c_double)]


class TraceJob:
    """one rv32im segment's preflight trace as the segment pipeline takes it (r0hip_trace_input):
    the global vector, the injector (index / offsets / Montgomery values), the cycle and
    transaction records, the BigInt bytes and backs. The arrays are kept as given (page-locked
    views from host_array() copy at full PCIe rate; others are staged)."""

    def __init__(self, glob, inj_index, inj_offsets, inj_values, cycles, txns, table_split, bigint=None,
                 bigint_records=None, mode=0):
        u = lambda a: a if isinstance(a, np.ndarray) and a.dtype == np.uint32 and a.flags.c_contiguous \
            else np.ascontiguousarray(a, dtype=np.uint32)
        self.glob, self.index, self.offsets, self.values = u(glob), u(inj_index), u(inj_offsets), u(inj_values)
        self.cycles, self.txns = np.ascontiguousarray(cycles), np.ascontiguousarray(txns)
        self.table_split = table_split
        self.bigint = None if bigint is None or not len(bigint) else np.ascontiguousarray(bigint, dtype=np.uint8)
        self.records = bigint_records
        self.backs = bigint_backs(bigint_records)
        pf = RawPreflightTrace(self.cycles.ctypes.data, self.txns.ctypes.data if self.txns.nbytes else None,
                               None if self.bigint is None else self.bigint.ctypes.data, self.txns.nbytes // 20,
                               0 if self.bigint is None else self.bigint.size, table_split)
        self.struct = TraceInput(mode, self.glob.ctypes.data, self.index.ctypes.data, self.index.size - 1,
                                 self.offsets.ctypes.data if self.offsets.size else None,
                                 self.values.ctypes.data if self.values.size else None, pf)

    def h2d_bytes(self):
        return sum(a.nbytes for a in (self.glob, self.index, self.offsets, self.values, self.cycles, self.txns)) + \
            (0 if self.bigint is None else self.bigint.nbytes)


def host_array(shape, dtype):
    """a numpy array over page-locked host memory (r0hip_host_alloc); the block goes back with
    r0hip_host_free when the last view of it is gone"""
    dtype = np.dtype(dtype)
    count = int(np.prod(shape))
    nbytes = max(1, count * dtype.itemsize)
    p = C.c_void_p()
    check(lib().r0hip_host_alloc(C.byref(p), nbytes))
    block = (C.c_uint8 * nbytes).from_address(p.value)
    block._owner = _HostBlock(p.value)  # the ctypes array is every view's base
    return np.frombuffer(block, dtype=dtype, count=count).reshape(shape)


def pinned_copy(a):
    """a copy of `a` in page-locked host memory (host_array)"""
    a = np.ascontiguousarray(a)
    out = host_array(a.shape, a.dtype)
    out[...] = a
    return out


class _HostBlock:
    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        if self.ptr:
            lib().r0hip_host_free(C.c_void_p(self.ptr))
            self.ptr = None


VERIFY_RECEIPTS_DEVICE = 2  # R0HIP_VERIFY_RECEIPTS_DEVICE


def _verify_mode(verify):
    """The pipelines' `verify` argument: "device" or 2 asks for the receipt check with the seal's
    Merkle openings hashed on the device; anything else is its truth value (True passes 1)."""
    if isinstance(verify, str):
        if verify not in ("host", "device"):
            raise ValueError(f"verify = {verify!r}: expected a bool, 2, \"host\" or \"device\"")
        return VERIFY_RECEIPTS_DEVICE if verify == "device" else 1
    if verify is not True and verify is not False and verify == VERIFY_RECEIPTS_DEVICE:
        return VERIFY_RECEIPTS_DEVICE
    return int(bool(verify))


def prove_trace_segments(hal, po2, traces, in_flight=2, seal_cap=1 << 22, verify=True, per_job=False):
    """The GPU worker unit (r0hip_prove_trace_segments): each TraceJob is one rv32im prove_core
    from its preflight trace; an uploader copies the traces into in_flight + 1 device trace sets
    while in_flight provers run, and (verify) every seal is checked by the native verifier, the
    validity equation included, on a host thread beside the proofs (verify="device" or 2: with the
    seal's Merkle openings hashed on the device, _verify_mode). Returns [(seal, mix)] in job
    order and raises on any failed job; per_job=True returns [(seal, mix, error or None,
    verify_ms, prove_ms)] instead, without raising for a job's own failure (prove_ms: from a
    prover taking the job to its seal in host memory)."""
    jobs = (TraceJobStruct * len(traces))()
    seals, mixes, keep = [], [], []
    for j, t in zip(jobs, traces):
        keep.append(t)
        j.trace = t.struct
        if t.backs is not None:
            j.h_bigint, j.n_bigint = C.cast(t.backs, C.c_void_p).value, len(t.backs)
        seals.append(np.zeros(seal_cap, dtype=np.uint32))
        mixes.append(np.zeros(36, dtype=np.uint32))
        j.h_seal, j.seal_cap, j.h_mix_out = seals[-1].ctypes.data, seal_cap, mixes[-1].ctypes.data
    err = lib().r0hip_prove_trace_segments(hal.suite, po2, C.cast(jobs, C.c_void_p), len(traces), in_flight,
                                           _verify_mode(verify))
    errors = []
    for j in jobs:
        errors.append(C.cast(j.error, C.c_char_p).value.decode() if j.error else None)
        if j.error:
            libc_free(j.error)
    if per_job:
        if err and not any(errors):
            check(err)  # a failure of the call itself, not of a job
        elif err:
            libc_free(err)
        return [(seal[: j.seal_len].copy(), mix, e, j.verify_ms, j.prove_ms) for j, seal, mix, e in zip(jobs, seals, mixes, errors)]
    check(err)
    if verify:
        assert all(j.verified for j in jobs)
    return [(seal[: j.seal_len].copy(), mix) for j, seal, mix in zip(jobs, seals, mixes)]


class RecursionInput(C.Structure):
    """struct r0hip_recursion_input (include/r0hip.h): one recursion job's host arrays"""
    _fields_ = [("h_ctrl", C.c_void_p), ("h_wom", C.c_void_p), ("n_wom", C.c_size_t), ("h_cycles", C.c_void_p),
                ("n_cycles", C.c_size_t), ("h_iops", C.c_void_p), ("n_iops", C.c_size_t),
                ("h_code_roots", C.c_void_p), ("n_code_roots", C.c_size_t)]


class WorkerJobStruct(C.Structure):
    """struct r0hip_worker_job (include/r0hip.h)"""
    _fields_ = [("kind", C.c_uint32), ("suite", C.c_int), ("po2", C.c_uint32), ("trace", TraceInput),
                ("h_bigint", C.c_void_p), ("n_bigint", C.c_size_t), ("recursion", RecursionInput),
                ("user", C.c_void_p), ("h_seal", C.c_void_p), ("seal_cap", C.c_size_t), ("seal_len", C.c_size_t),
                ("h_mix_out", C.c_void_p), ("error", C.c_void_p), ("verified", C.c_int), ("verify_ms", C.c_double),
                ("prove_ms", C.c_double), ("ticket", C.c_uint64), ("backs", C.c_void_p)]


class WorkerProgramJobStruct(C.Structure):
    """struct r0hip_worker_program_job (include/r0hip.h): a kind-3 job, the job struct with the
    resident program's handle appended; its `job` member is what submit takes"""
    _fields_ = [("job", WorkerJobStruct), ("program", C.c_void_p)]


class WorkerInputJobStruct(C.Structure):
    """struct r0hip_worker_input_job (include/r0hip.h): a kind-4 job, the job struct followed by
    the resident program's handle and the input words; its `job` member is what submit takes"""
    _fields_ = [("job", WorkerJobStruct), ("program", C.c_void_p), ("h_input", C.c_void_p), ("n_input", C.c_size_t),
                ("h_output", C.c_void_p), ("output_cap", C.c_size_t), ("n_output", C.c_size_t)]


class WorkerStats(C.Structure):
    """struct r0hip_worker_stats (include/r0hip.h): which way the worker's kind-4 preflights went"""
    _fields_ = [("preflight_threads", C.c_uint32), ("preflight_slots", C.c_uint32),
                ("peak_slots_in_use", C.c_uint32), ("reserved", C.c_uint32), ("pool_jobs", C.c_uint64),
                ("inline_jobs", C.c_uint64), ("slot_bytes", C.c_uint64), ("pool_busy_ms", C.c_double),
                ("uploader_preflight_ms", C.c_double), ("uploader_wait_preflight_ms", C.c_double)]


JOB_RV32IM_TRACE, JOB_RECURSION, JOB_RV32IM_BACKS, JOB_RECURSION_PROGRAM, JOB_RECURSION_INPUT = 0, 1, 2, 3, 4


class BacksJob:
    """one rv32im segment as the worker's kind-2 job takes it: the global vector, the injector
    as a Backs, the cycle and transaction records and the BigInt bytes. No injector arrays and
    no BigInt records: both come from the Back records. Arrays are kept as given."""

    def __init__(self, glob, backs, cycles, txns, table_split, bigint=None, mode=0):
        self.glob = glob if isinstance(glob, np.ndarray) and glob.dtype == np.uint32 and glob.flags.c_contiguous \
            else np.ascontiguousarray(glob, dtype=np.uint32)
        self.backs = backs
        self.cycles, self.txns = np.ascontiguousarray(cycles), np.ascontiguousarray(txns)
        self.bigint = None if bigint is None or not len(bigint) else np.ascontiguousarray(bigint, dtype=np.uint8)
        pf = RawPreflightTrace(self.cycles.ctypes.data, self.txns.ctypes.data if self.txns.nbytes else None,
                               None if self.bigint is None else self.bigint.ctypes.data, self.txns.nbytes // 20,
                               0 if self.bigint is None else self.bigint.size, table_split)
        self.struct = TraceInput(mode, self.glob.ctypes.data, None, 0, None, None, pf)

    def h2d_bytes(self):
        return sum(a.nbytes for a in (self.glob, self.cycles, self.txns)) + self.backs.nbytes() + \
            (0 if self.bigint is None else self.bigint.nbytes)


class Worker:
    """The GPU worker (r0hip_worker_*): a persistent queue that takes rv32im trace jobs of any
    po2 <= max_po2 and recursion jobs as they arrive, proves them pipelined over `in_flight`
    provers, checks every receipt (verify) and hands the results back in completion order.

        with Worker(hal, max_po2=20, in_flight=3) as w:
            t0 = w.submit_trace(job, 20)
            t1 = w.submit_recursion(17, ctrl, wom, cycles, iops, code_roots=roots)
            ticket, seal, mix, error, verify_ms, prove_ms = w.wait(10.0)

    noise_key (8 words or 32 bytes) makes the recursion jobs' ZK noise reproducible and is for
    tests only: the default (None) draws an OS key for the worker's lifetime. The inputs of a
    job are kept alive here until wait() returns it. Leaving the `with` block destroys the
    worker, which first runs everything submitted to completion."""

    def __init__(self, hal, max_po2, in_flight=2, verify=True, noise_key=None, seal_cap=1 << 22):
        self.hal, self.verify, self.seal_cap = hal, _verify_mode(verify), seal_cap  # 0, 1 or 2 ("device")
        self._pending = {}  # address of the job struct -> (struct, seal, mix, inputs)
        self.outputs = {}  # ticket of a returned kind-4 job -> Preflight.output, until output() reads it
        k, kp = _key_words(noise_key)
        h = C.c_void_p()
        check(lib().r0hip_worker_create(C.byref(h), max_po2, in_flight, int(self.verify), kp))
        self._h = h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def close(self):
        """r0hip_worker_destroy: run what was submitted, join the threads, free the sets. Results
        not yet waited for are dropped (their error strings are freed)."""
        h, self._h = getattr(self, "_h", None), None
        if h is None or not h.value:
            return
        err = lib().r0hip_worker_destroy(h)
        for job, _seal, _mix, _keep in self._pending.values():
            if job.error:
                libc_free(job.error)
        self._pending.clear()
        self.outputs.clear()
        check(err)

    def _handle(self):
        if self._h is None or not self._h.value:
            raise R0HipError("the worker is closed")
        return self._h

    def set_witness_check(self, on):
        """r0hip_worker_set_witness_check: the jobs submitted from now on are checked (or not) as
        set_witness_check checks a proof; a violated job fails alone with the check's message"""
        check(lib().r0hip_worker_set_witness_check(self._handle(), 1 if on else 0))

    def set_preflight_threads(self, n):
        """r0hip_worker_set_preflight_threads: kind-4 preflights on n pool threads (1..8) ahead of
        the uploader, or on the uploader thread itself (0, the default). Refused (R0HipError) above
        8 and while a job is outstanding. Returns the previous n."""
        was = C.c_uint32()
        check(lib().r0hip_worker_set_preflight_threads(self._handle(), n, C.byref(was)))
        return int(was.value)

    def stats(self):
        """r0hip_worker_get_stats as a WorkerStats: pool_jobs and inline_jobs tell which thread ran
        each kind-4 preflight, uploader_wait_preflight_ms whether the uploader still waits"""
        st = WorkerStats()
        check(lib().r0hip_worker_get_stats(self._handle(), C.byref(st), C.sizeof(st)))
        return st

    def _submit(self, job, mix_words, keep):
        seal = np.zeros(self.seal_cap, dtype=np.uint32)
        mix = np.zeros(mix_words, dtype=np.uint32)
        job.h_seal, job.seal_cap, job.h_mix_out = seal.ctypes.data, self.seal_cap, mix.ctypes.data
        check(lib().r0hip_worker_submit(self._handle(), C.byref(job)))
        self._pending[C.addressof(job)] = (job, seal, mix, keep)
        return int(job.ticket)

    def submit_trace(self, trace, po2, suite=None):
        """queue one rv32im prove_core from a TraceJob at segment size 2^po2; returns its ticket"""
        job = WorkerJobStruct()
        job.kind, job.po2 = JOB_RV32IM_TRACE, po2
        job.suite = self.hal.suite if suite is None else (SUITES[suite] if isinstance(suite, str) else int(suite))
        job.trace = trace.struct
        if trace.backs is not None:
            job.h_bigint, job.n_bigint = C.cast(trace.backs, C.c_void_p).value, len(trace.backs)
        return self._submit(job, 36, trace)

    def submit_backs(self, job, po2, suite=None):
        """queue one rv32im prove_core from a BacksJob (kind R0HIP_JOB_RV32IM_BACKS) at segment
        size 2^po2; returns its ticket. A bad record is refused here (R0HipError)."""
        wj = WorkerJobStruct()
        wj.kind, wj.po2 = JOB_RV32IM_BACKS, po2
        wj.suite = self.hal.suite if suite is None else (SUITES[suite] if isinstance(suite, str) else int(suite))
        wj.trace = job.struct
        wj.backs = None if job.backs is None else C.addressof(job.backs.struct)
        return self._submit(wj, 36, job)

    def submit_recursion(self, po2, ctrl, wom, cycles, iops, code_roots=None, suite=None):
        """queue one recursion proof from the program's control group (23 x 2^po2 host words)
        and its preflight; code_roots: the allow-list (8 words each) its receipt check applies.
        Returns its ticket, which is also the stream_id of its ZK noise."""
        w, c, i = _trace(wom, cycles, iops)
        ct = ctrl if isinstance(ctrl, np.ndarray) and ctrl.dtype == np.uint32 and ctrl.flags.c_contiguous \
            else np.ascontiguousarray(ctrl, dtype=np.uint32)
        if ct.size != 23 << po2:
            raise R0HipError(f"the control group of a po2={po2} recursion job is {23 << po2} words, got {ct.size}")
        roots = np.ascontiguousarray(np.zeros(0, np.uint32) if code_roots is None else code_roots,
                                     dtype=np.uint32).reshape(-1)
        if roots.size % 8:
            raise R0HipError("code_roots holds 8 words per root")
        job = WorkerJobStruct()
        job.kind, job.po2 = JOB_RECURSION, po2
        job.suite = self.hal.suite if suite is None else (SUITES[suite] if isinstance(suite, str) else int(suite))
        job.recursion = RecursionInput(ct.ctypes.data, w.ctypes.data if w.size else None, w.size // 4,
                                       c.ctypes.data if c.size else None, c.size // 2,
                                       i.ctypes.data if i.size else None, i.size // 4,
                                       roots.ctypes.data if roots.size else None, roots.size // 8)
        return self._submit(job, 20, (ct, w, c, i, roots))

    def submit_recursion_program(self, program, wom, cycles, iops, code_roots=None, po2=None, suite=None):
        """queue one recursion proof from a RecursionProgram (kind R0HIP_JOB_RECURSION_PROGRAM):
        no control group is staged. code_roots: the allow-list of its receipt check (default:
        the program's own control id). po2 and suite default to the program's; a mismatch is
        refused (R0HipError). Returns its ticket, which is also the stream_id of its ZK noise."""
        w, c, i = _trace(wom, cycles, iops)
        roots = np.ascontiguousarray(np.zeros(0, np.uint32) if code_roots is None else code_roots,
                                     dtype=np.uint32).reshape(-1)
        if roots.size % 8:
            raise R0HipError("code_roots holds 8 words per root")
        p_suite, p_po2 = program.info()[:2]
        pj = WorkerProgramJobStruct()
        pj.program = program._handle().value
        job = pj.job  # a view of pj's first member: the address submit takes and wait returns
        job.kind, job.po2 = JOB_RECURSION_PROGRAM, p_po2 if po2 is None else po2
        job.suite = p_suite if suite is None else (SUITES[suite] if isinstance(suite, str) else int(suite))
        job.recursion = RecursionInput(None, w.ctypes.data if w.size else None, w.size // 4,
                                       c.ctypes.data if c.size else None, c.size // 2,
                                       i.ctypes.data if i.size else None, i.size // 4,
                                       roots.ctypes.data if roots.size else None, roots.size // 8)
        return self._submit(job, 20, (pj, program, w, c, i, roots))

    def submit_recursion_input(self, program, inp, code_roots=None, po2=None, suite=None, prepare=True,
                               output_cap=None):
        """queue one recursion proof from a RecursionProgram and the reference's `input` (kind
        R0HIP_JOB_RECURSION_INPUT): the preflight runs on the worker's uploader thread, or on a
        pool thread after set_preflight_threads. Returns its ticket; output(ticket) gives
        Preflight.output once wait() has returned the job. prepare=False leaves a program without
        a plan as it is (the worker makes the plan; the output buffer then needs output_cap, its
        size in words, which also overrides the prepared program's own count)."""
        x = np.ascontiguousarray(inp, dtype=np.uint32).reshape(-1)
        roots = np.ascontiguousarray(np.zeros(0, np.uint32) if code_roots is None else code_roots,
                                     dtype=np.uint32).reshape(-1)
        if roots.size % 8:
            raise R0HipError("code_roots holds 8 words per root")
        p_suite, p_po2 = program.info()[:2]
        if prepare and not program.input_info().prepared:
            program.prepare_input()
        cap = program.input_info().n_output if output_cap is None else int(output_cap)
        out = np.zeros(cap + 1, dtype=np.uint32)
        ij = WorkerInputJobStruct()
        ij.program = program._handle().value
        ij.h_input, ij.n_input = x.ctypes.data if x.size else None, x.size
        ij.h_output, ij.output_cap = out.ctypes.data, out.size - 1
        job = ij.job
        job.kind, job.po2 = JOB_RECURSION_INPUT, p_po2 if po2 is None else po2
        job.suite = p_suite if suite is None else (SUITES[suite] if isinstance(suite, str) else int(suite))
        job.recursion = RecursionInput(None, None, 0, None, 0, None, 0, roots.ctypes.data if roots.size else None,
                                       roots.size // 8)
        return self._submit(job, 20, (ij, program, x, out, roots))

    def output(self, ticket):
        """Preflight.output of a kind-4 job that wait() has returned (kept for the last 256 such
        jobs, until it is read)"""
        return self.outputs.pop(ticket)

    def outstanding(self):
        """jobs submitted and not yet returned by wait()"""
        return len(self._pending)

    def wait(self, timeout_s=None):
        """The next finished job in completion order as (ticket, seal, mix, error or None,
        verify_ms, prove_ms), or None when the timeout passed (None waits without limit, 0
        polls) or nothing is outstanding. With verify, a job without an error that the
        verifier did not pass raises R0HipError."""
        done = C.c_void_p()
        ms = -1 if timeout_s is None else max(0, int(round(timeout_s * 1000)))
        check(lib().r0hip_worker_wait(self._handle(), C.byref(done), ms))
        if not done.value:
            return None
        entry = self._pending.pop(done.value, None)
        if entry is None:
            raise R0HipError("r0hip_worker_wait returned a job this Worker did not submit")
        job, seal, mix, keep = entry
        if job.kind == JOB_RECURSION_INPUT:
            self.outputs[int(job.ticket)] = keep[3][: keep[0].n_output].copy()
            while len(self.outputs) > 256:
                self.outputs.pop(next(iter(self.outputs)))
        error = None
        if job.error:
            error = C.cast(job.error, C.c_char_p).value.decode()
            libc_free(job.error)
            job.error = None
        if self.verify and error is None and not job.verified:
            raise R0HipError(f"job {job.ticket} came back without an error and without a verified receipt")
        return int(job.ticket), seal[: job.seal_len].copy(), mix, error, job.verify_ms, job.prove_ms


def prove_segments(hal, circuit, po2, witnesses, version=None, in_flight=2, seal_cap=1 << 24):
    """The native segment pipeline (r0hip_prove_segments): `witnesses` is a list of
    (code, data, accum, global) host arrays (numpy uint32, ideally views of page-locked
    memory) or raw host pointers; returns [(seal, mix)] in job order. For rv32im, accum may
    be None: the prover then runs the accumulation on the device (r0hip_prove_segment_accum's
    path) and nothing of that group crosses PCIe; a 5th element then gives the job's BigInt
    backs [(row, poly_op, coeff, bytes16)]."""
    mix_size = circuit_info(circuit)["mix_size"]  # any circuit the library knows, registered ones included
    jobs = (SegmentJob * len(witnesses))()
    keep, seals, mixes = [], [], []
    for j, w in zip(jobs, witnesses):
        ptrs = []
        backs = bigint_backs(w[4]) if len(w) > 4 else None
        if backs is not None:
            keep.append(backs)
            j.h_bigint, j.n_bigint = C.cast(backs, C.c_void_p).value, len(backs)
        for a in w[:4]:
            if isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a, dtype=np.uint32)
                keep.append(a)
                ptrs.append(a.ctypes.data)
            else:
                ptrs.append(0 if a is None else int(a))
        j.h_code, j.h_data, j.h_accum, j.h_global = ptrs
        seals.append(np.zeros(seal_cap, dtype=np.uint32))
        mixes.append(np.zeros(mix_size, dtype=np.uint32))
        j.h_seal, j.seal_cap, j.h_mix_out = seals[-1].ctypes.data, seal_cap, mixes[-1].ctypes.data
    err = lib().r0hip_prove_segments(circuit.encode(), hal.suite, po2, int(version is not None), version or 0,
                                     C.cast(jobs, C.c_void_p), len(witnesses), in_flight)
    for j in jobs:
        if j.error:
            libc_free(j.error)
    check(err)
    return [(seal[: j.seal_len].copy(), mix) for j, seal, mix in zip(jobs, seals, mixes)]


class Opening(C.Structure):
    """struct r0hip_opening (include/r0hip.h): one Merkle opening over a word buffer"""
    _fields_ = [("row_off", C.c_uint64), ("path_off", C.c_uint64), ("index", C.c_uint64), ("cols", C.c_uint32),
                ("levels", C.c_uint32)]


def merkle_open_digests(suite, words, openings):
    """r0hip_merkle_open_digests: the device step of the receipt check by itself. `openings` is a
    list of (row_off, path_off, index, cols, levels) over the u32 array `words`; returns
    (digests [n, 8], status [n]): per opening the row hash folded up its path, and 0 or 2 (a
    Poseidon2 path digest word >= p). Suites Poseidon2 and SHA-256, and Poseidon254 while
    set_verify_device_poseidon254(1) holds."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    sid = SUITES[suite] if isinstance(suite, str) else suite
    n = len(openings)
    table = (Opening * max(n, 1))()
    for t, o in zip(table, openings):
        t.row_off, t.path_off, t.index, t.cols, t.levels = (int(v) for v in o)
    digests, status = np.zeros((n, 8), np.uint32), np.zeros(n, np.uint32)
    check(lib().r0hip_merkle_open_digests(sid, words.ctypes.data_as(u32p), words.size, C.cast(table, C.c_void_p), n,
                                          digests.ctypes.data_as(u32p), status.ctypes.data_as(u32p)))
    return digests, status


def set_verify_device_poseidon254(on):
    """r0hip_set_verify_device_poseidon254: process-wide and off by default. While on, a device
    receipt check (verify_seal(where="device"), verify=2 in the pipelines and the worker) and
    merkle_open_digests take Poseidon254 openings on the GPU as well; verdicts and messages are the
    host check's. `on` is 0 or 1 (False or True); needs no GPU."""
    check(lib().r0hip_set_verify_device_poseidon254(int(on)))


VERIFY_WHERE = {"host": 0, "device": 1}  # R0HIP_VERIFY_HOST, R0HIP_VERIFY_DEVICE


def verify_seal(circuit, suite, seal, check_validity=True, code_roots=None, return_code_root=False, where="host"):
    """r0hip_verify_seal: the native seal verifier (host-only, no GPU; where="device": the same
    check through r0hip_verify_seal_on with the seal's Merkle openings hashed on the GPU); returns the
    segment po2 (and the code root, 8 words, with return_code_root), raises R0HipError
    naming the failed check. code_roots: allowed code/control roots (check_code,
    zkp/src/verify/mod.rs:531). check_validity=False calls the test-only
    r0hip_testing_verify_seal_structure instead (no constraint equation, no code-root check),
    for seals of synthetic witnesses."""
    seal = np.ascontiguousarray(seal, dtype=np.uint32)
    po2 = C.c_uint32(0)
    sid = SUITES[suite] if isinstance(suite, str) else suite
    on = VERIFY_WHERE[where] if isinstance(where, str) else int(where)
    if not check_validity:
        assert code_roots is None and not return_code_root, "the structure check binds no code root"
        if on != 0:
            check(lib().r0hip_testing_verify_seal_structure_on(on, circuit.encode(), sid, seal.ctypes.data_as(u32p),
                                                               seal.size, C.byref(po2)))
            return po2.value
        check(lib().r0hip_testing_verify_seal_structure(circuit.encode(), sid, seal.ctypes.data_as(u32p), seal.size,
                                                        C.byref(po2)))
        return po2.value
    roots = np.ascontiguousarray(np.zeros(0, np.uint32) if code_roots is None else code_roots, dtype=np.uint32)
    assert roots.size % 8 == 0
    root_out = np.zeros(8, np.uint32)
    if on != 0:
        check(lib().r0hip_verify_seal_on(on, circuit.encode(), sid, seal.ctypes.data_as(u32p), seal.size,
                                         roots.ctypes.data_as(u32p), roots.size // 8, root_out.ctypes.data_as(u32p),
                                         C.byref(po2)))
        return (po2.value, root_out) if return_code_root else po2.value
    check(lib().r0hip_verify_seal(circuit.encode(), sid, seal.ctypes.data_as(u32p), seal.size,
                                  roots.ctypes.data_as(u32p), roots.size // 8, root_out.ctypes.data_as(u32p),
                                  C.byref(po2)))
    return (po2.value, root_out) if return_code_root else po2.value


def poly_ext(circuit, mix, glob, eval_u, poly_mix):
    """r0hip_poly_ext (host-only): Montgomery words in, the FpExt result as 4 Montgomery words."""
    arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (mix, glob, eval_u, poly_mix)]
    out = np.zeros(4, np.uint32)
    check(lib().r0hip_poly_ext(circuit.encode(), *(a.ctypes.data_as(u32p) for a in arrs), out.ctypes.data_as(u32p)))
    return out


class ConstraintReport(C.Structure):
    """struct r0hip_constraint_report"""
    _fields_ = [("bad_rows", C.c_uint64), ("first_row", C.c_uint32), ("first_term", C.c_int32),
                ("n_rows", C.c_uint32), ("rows", C.c_uint32 * 16)]


def constraint_rows(circuit, po2, code, data, accum, mix, glob, poly_mix=None, out=None):
    """r0hip_constraint_rows: the circuit's constraint polynomial on the 2^po2 rows of the witness
    groups (device Buffers, as prove_segment takes them; mix and glob device Buffers as eval_check
    takes them). poly_mix: 4 Montgomery words, None draws them from the OS. out: an optional
    Buffer of 2^po2 FpExt that receives every row's value. Returns a dict: bad_rows, first_row
    (None if no row is bad), first_term (the .poly.ir id, None if no row is bad) and rows (the
    first 16 bad rows, ascending). A violated witness is a result, not an error."""
    rep = ConstraintReport()
    pm = None if poly_mix is None else np.ascontiguousarray(poly_mix, dtype=np.uint32)
    ptr = lambda b: None if b is None else C.c_void_p(b.ptr if isinstance(b, Buffer) else b)
    check(lib().r0hip_constraint_rows(circuit.encode() if circuit is not None else None, po2, ptr(code), ptr(data),
                                      ptr(accum), ptr(mix), ptr(glob),
                                      None if pm is None else pm.ctypes.data_as(u32p), ptr(out), C.byref(rep)))
    bad = int(rep.bad_rows)
    return {"bad_rows": bad, "first_row": int(rep.first_row) if bad else None,
            "first_term": int(rep.first_term) if bad else None, "rows": [int(r) for r in rep.rows[:rep.n_rows]]}


def constraint_term(circuit, taps, mix, glob, poly_mix):
    """r0hip_constraint_term (host-only, no GPU): the id in <circuit>.poly.ir of the first term
    that one row's tap values (Montgomery words, tap order) violate, or None if there is none."""
    arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32) for a in (taps, mix, glob, poly_mix)]
    term = C.c_int32(-1)
    check(lib().r0hip_constraint_term(circuit.encode() if circuit is not None else None,
                                      *(None if a is None else a.ctypes.data_as(u32p) for a in arrs), C.byref(term)))
    return None if term.value < 0 else int(term.value)


def set_witness_check(on):
    """r0hip_set_witness_check: while on, the provers of the calling thread check the constraint
    polynomial on the trace rows before the accum commit and raise R0HipError("constraint check
    failed: K of N rows, first at cycle R (term T)") instead of proving a violated witness.
    Returns the previous mode."""
    was = C.c_int(0)
    check(lib().r0hip_set_witness_check(1 if on else 0, C.byref(was)))
    return bool(was.value)


def libc_free(p):
    C.CDLL(None).free(C.c_void_p(p))


def last_profile():
    buf = C.create_string_buffer(4096)
    check(lib().r0hip_last_profile(buf, 4096))
    out = {}
    for kv in buf.value.decode().split(";"):
        if "=" in kv:
            k, v = kv.split("=")
            out[k] = float(v)
    return out


def set_kernel_timing(on):
    check(lib().r0hip_set_kernel_timing(int(bool(on))))


def kernel_times():
    """{kernel: (total_ms, calls, algorithmic_bytes, modmul_equivalents)} since timing was enabled."""
    buf = C.create_string_buffer(16384)
    check(lib().r0hip_kernel_times(buf, 16384))
    out = {}
    for kv in buf.value.decode().split(";"):
        if "=" in kv:
            k, v = kv.split("=")
            ms, calls, b, mm = v.split(":")
            out[k] = (float(ms), int(calls), float(b), float(mm))
    return out


def eval_check_launched():
    """(launched, kernels) of the calling thread's last eval_check or constraint-rows check
    (r0hip_eval_check_launched): how many of the program's kernels ran after the zero scan of the
    selector columns."""
    out = (C.c_int * 2)()
    check(lib().r0hip_eval_check_launched(out))
    return int(out[0]), int(out[1])


def zero_scan(matrix, cols, words):
    """r0hip_testing_zero_scan: the mask of the all-zero columns (bit c) among `cols` columns of `words`
    words, laid one after the other from `matrix` (a Buffer or a device address)."""
    mask = C.c_uint64(0)
    check(lib().r0hip_testing_zero_scan(C.c_void_p(matrix.ptr if isinstance(matrix, Buffer) else matrix), cols, words,
                                C.byref(mask)))
    return int(mask.value)


def call_stats():
    """The calling thread's device entry-point calls (r0hip_call_stats): how many were made, how
    many drained the stream before returning, how many returned with their work only queued."""
    out = (C.c_uint64 * 3)()
    check(lib().r0hip_call_stats(out))
    return {"calls": int(out[0]), "drained": int(out[1]), "queued": int(out[2])}


def set_proof_streams(n):
    """r0hip_set_proof_streams: how many streams one proof of the calling thread may use (1, the
    default, to 3). With n >= 2 the code group's commitment runs on a side stream, beside the
    witness generation (prove_recursion*) or the data group's commitment; the seal is the same
    words. For a caller that proves one task at a time; a pipeline or a worker fills the chip
    with other segments and runs at 1. Returns the previous value."""
    was = C.c_uint32(0)
    check(lib().r0hip_set_proof_streams(C.c_uint32(n), C.byref(was)))
    return int(was.value)


def mem_stats():
    """The library's MemoryTracker (zkp/src/hal/mod.rs:292-317): live and reserved device
    bytes, their peaks since mem_reset_peak(), and how many hipMalloc calls it has made."""
    out = (C.c_uint64 * 5)()
    check(lib().r0hip_mem_stats(out))
    return dict(zip(("live", "peak_live", "reserved", "peak_reserved", "mallocs"), (int(x) for x in out)))


def mem_reset_peak():
    check(lib().r0hip_mem_reset_peak())


def trim():
    """r0hip_trim: release idle pooled device memory (this thread's and exited threads')."""
    check(lib().r0hip_trim())
