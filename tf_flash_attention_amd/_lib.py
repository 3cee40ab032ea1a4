"""ctypes binding to the C ABI in ``include/fa_api.h`` (libfa_hip.so).

This is the only way the Python layer reaches the device: there is no eager /
CPU fallback.  If the HIP library is missing the first call raises
:class:`LibraryNotBuiltError` — loudly, by design.
"""

from __future__ import annotations

import contextlib
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FA_HIP_LIB", os.path.join(_HERE, "libfa_hip.so"))

F16, F32, F64 = 0, 1, 2
FULL, CAUSAL, LOCAL = 0, 1, 2
NONE_FRONT, SCALE_FRONT, SCALE_END = 0, 1, 2

FA_OK = 0
FA_ERR_INVALID_ARGUMENT = -1
FA_ERR_UNSUPPORTED = -2
FA_ERR_WORKSPACE_TOO_SMALL = -3
FA_MAX_PARTS = 8

# every symbol include/fa_api.h declares (checked by tests/test_boundary.py)
EXPORTED_SYMBOLS = (
    "fa_sync_mode_from_string",
    "fa_validate",
    "fa_forward",
    "fa_forward_workspace_bytes",
    "fa_forward_ws",
    "fa_forward_split_plan",
    "fa_forward_grouped_plan",
    "fa_forward_grouped_workspace_bytes",
    "fa_forward_grouped",
    "fa_forward_ragged_plan",
    "fa_forward_ragged_workspace_bytes",
    "fa_forward_ragged",
    "fa_forward_paged_plan",
    "fa_forward_paged_workspace_bytes",
    "fa_forward_paged",
    "fa_forward_ragged_fp8",
    "fa_forward_paged_fp8",
    "fa_forward_ragged_window_plan",
    "fa_forward_paged_window_plan",
    "fa_forward_ragged_window_workspace_bytes",
    "fa_forward_paged_window_workspace_bytes",
    "fa_forward_ragged_window",
    "fa_forward_paged_window",
    "fa_forward_ragged_window_fp8",
    "fa_forward_paged_window_fp8",
    "fa_forward_ragged_prefill_plan",
    "fa_forward_paged_prefill_plan",
    "fa_forward_ragged_prefill_workspace_bytes",
    "fa_forward_paged_prefill_workspace_bytes",
    "fa_forward_ragged_prefill",
    "fa_forward_paged_prefill",
    "fa_forward_ragged_prefill_fp8",
    "fa_forward_paged_prefill_fp8",
    "fa_forward_ragged_tree_plan",
    "fa_forward_paged_tree_plan",
    "fa_forward_ragged_tree_workspace_bytes",
    "fa_forward_paged_tree_workspace_bytes",
    "fa_forward_ragged_tree",
    "fa_forward_paged_tree",
    "fa_forward_ragged_tree_fp8",
    "fa_forward_paged_tree_fp8",
    "fa_forward_ragged_window_prefill_plan",
    "fa_forward_paged_window_prefill_plan",
    "fa_forward_ragged_window_prefill_workspace_bytes",
    "fa_forward_paged_window_prefill_workspace_bytes",
    "fa_forward_ragged_window_prefill",
    "fa_forward_paged_window_prefill",
    "fa_forward_ragged_window_prefill_fp8",
    "fa_forward_paged_window_prefill_fp8",
    "fa_append_ragged",
    "fa_append_paged",
    "fa_append_ragged_fp8",
    "fa_append_paged_fp8",
    "fa_backward_workspace_bytes",
    "fa_backward",
    "fa_backward_split_plan",
    "fa_backward_split_q_plan",
    "fa_backward_split_workspace_bytes",
    "fa_backward_split",
    "fa_merge_partials",
    "fa_accumulate_parts",
    "fa_estimate_forward_flops",
    "fa_allowed_pairs",
    "fa_error_string",
    "fa_last_error",
    "fa_build_info",
    "fa_rule_mask",
    "fa_rule_probe",
    "fa_forward_kernel",
)


DECODE_CACHES = ("ragged", "paged")
DECODE_FORMS = ("plain", "window", "prefill", "tree", "window_prefill")


def decode_entry_points(cache, form, fp8):
    """The (plan, workspace_bytes, forward) entry-point names of the decode forward over ``cache`` (of
    DECODE_CACHES) in ``form`` (of DECODE_FORMS); an FP8 cache shares the plan and workspace of the fp16 one."""
    if cache not in DECODE_CACHES or form not in DECODE_FORMS:
        raise ValueError(f"no decode forward over cache {cache!r} in form {form!r}")
    stem = f"fa_forward_{cache}" + ("" if form == "plain" else f"_{form}")
    return stem + "_plan", stem + "_workspace_bytes", stem + ("_fp8" if fp8 else "")


def append_entry_point(cache, fp8):
    """The name of the fused K/V append into ``cache`` (of DECODE_CACHES)."""
    if cache not in DECODE_CACHES:
        raise ValueError(f"no append into cache {cache!r}")
    return f"fa_append_{cache}" + ("_fp8" if fp8 else "")


class LibraryNotBuiltError(RuntimeError):
    pass


class FaProblem(ctypes.Structure):
    _fields_ = [
        ("dtype", ctypes.c_int32),
        ("policy", ctypes.c_int32),
        ("seq_dims", ctypes.c_int32),
        ("sync_mode", ctypes.c_int32),
        ("b", ctypes.c_int64),
        ("q_seq", ctypes.c_int32 * 2),
        ("k_seq", ctypes.c_int32 * 2),
        ("d", ctypes.c_int32),
        ("v_d", ctypes.c_int32),
        ("window_size", ctypes.c_int32),
        ("log2_stride_size", ctypes.c_int32),
        ("is_causal", ctypes.c_int32),
    ]


_lock = threading.Lock()
_lib = None
_tls = threading.local()  # .override: a library routed in by using() on THIS thread (tests: the diag build)
# the library routed in by using() for the whole process: autograd runs a CUDA tensor's backward on
# its own device thread, which does not see the thread-local override of the thread that called
# .backward() (the diag-variant backward tests otherwise ran the product library)
_process_override = None
_process_owner = None   # thread ident of the using() block that set _process_override
_process_depth = 0
_loaded = {}
DIAG_LIB_PATH = os.path.join(_HERE, "libfa_hip_diag.so")


def _declare(lib):
    P = ctypes.POINTER(FaProblem)
    vp = ctypes.c_void_p
    lib.fa_sync_mode_from_string.argtypes = [ctypes.c_char_p]
    lib.fa_sync_mode_from_string.restype = ctypes.c_int
    lib.fa_validate.argtypes = [P]
    lib.fa_validate.restype = ctypes.c_int
    lib.fa_forward.argtypes = [vp, P, vp, vp, vp, vp, vp, vp]
    lib.fa_forward.restype = ctypes.c_int
    lib.fa_forward_workspace_bytes.argtypes = [P]
    lib.fa_forward_workspace_bytes.restype = ctypes.c_size_t
    lib.fa_forward_ws.argtypes = [vp, P, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    lib.fa_forward_ws.restype = ctypes.c_int
    lib.fa_forward_split_plan.argtypes = [P, ctypes.POINTER(ctypes.c_int32)]
    lib.fa_forward_split_plan.restype = ctypes.c_int
    lib.fa_backward_workspace_bytes.argtypes = [P]
    lib.fa_backward_workspace_bytes.restype = ctypes.c_size_t
    lib.fa_backward.argtypes = [vp, P, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    lib.fa_backward.restype = ctypes.c_int
    # (absent from a library built before the split-key backward: tools/lib_ab.py routes such a build in
    # through using() and calls fa_backward only; the wrappers fail loudly on the missing symbol)
    if hasattr(lib, "fa_backward_split"):
        lib.fa_backward_split_plan.argtypes = [P, ctypes.POINTER(ctypes.c_int32)]
        lib.fa_backward_split_plan.restype = ctypes.c_int
        lib.fa_backward_split_workspace_bytes.argtypes = [P]
        lib.fa_backward_split_workspace_bytes.restype = ctypes.c_size_t
        lib.fa_backward_split.argtypes = [vp, P, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
        lib.fa_backward_split.restype = ctypes.c_int
    # (absent from a library built before the split-query dK/dV pass, as above)
    if hasattr(lib, "fa_backward_split_q_plan"):
        lib.fa_backward_split_q_plan.argtypes = [P, ctypes.POINTER(ctypes.c_int32)]
        lib.fa_backward_split_q_plan.restype = ctypes.c_int
    # (absent from a library built before the merge of partials, as above)
    if hasattr(lib, "fa_merge_partials"):
        pp = ctypes.POINTER(vp)  # a host array of device pointers
        lib.fa_merge_partials.argtypes = [vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                          ctypes.c_int32, pp, pp, pp, vp, vp, vp]
        lib.fa_merge_partials.restype = ctypes.c_int
        lib.fa_accumulate_parts.argtypes = [vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, pp, vp]
        lib.fa_accumulate_parts.restype = ctypes.c_int
    # (absent from a library built before the grouped-query forward, as above)
    if hasattr(lib, "fa_forward_grouped"):
        lib.fa_forward_grouped_plan.argtypes = [P, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
        lib.fa_forward_grouped_plan.restype = ctypes.c_int
        lib.fa_forward_grouped_workspace_bytes.argtypes = [P, ctypes.c_int32]
        lib.fa_forward_grouped_workspace_bytes.restype = ctypes.c_size_t
        lib.fa_forward_grouped.argtypes = [vp, P, ctypes.c_int32, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
        lib.fa_forward_grouped.restype = ctypes.c_int
    # The decode forwards (include/fa_api.h): a cache times a form times the cache's precision, every argument
    # list made of the same pieces.  A paged cache adds (page) to the plan functions and (block_table, max_pages,
    # page, num_pages) to the forward, an FP8 cache (k_scale, v_scale) to the forward, a window `window` after the
    # plan functions' own arguments and where the forward's tail_causal stands, a tree the device mask's pointer
    # there.  (Each is absent from a library built before its feature, as above.)
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    for cache in DECODE_CACHES:
        for form in DECODE_FORMS:
            own = [P, i32] + ([i32] if cache == "paged" else []) + ([i32] if form in ("window", "window_prefill") else [])
            for fp8 in (False, True):
                plan, ws_bytes, forward = decode_entry_points(cache, form, fp8)
                if not hasattr(lib, forward):
                    continue
                getattr(lib, plan).argtypes = own + [ctypes.POINTER(i32)]
                getattr(lib, plan).restype = ctypes.c_int
                getattr(lib, ws_bytes).argtypes = own
                getattr(lib, ws_bytes).restype = ctypes.c_size_t
                getattr(lib, forward).argtypes = ([vp, P, i32, vp, vp, vp] + ([vp, vp] if fp8 else [])
                                                  + ([vp, i32, i32, i64] if cache == "paged" else [])
                                                  + [vp, i32, vp if form == "tree" else i32]
                                                  + [vp, vp, vp, vp, ctypes.c_size_t])
                getattr(lib, forward).restype = ctypes.c_int
    # The fused K/V appends (include/fa_api.h): the same pieces again, the caches written instead of read; (k_scale,
    # v_scale) after an FP8 cache, (block_table, max_pages, page, num_pages) after a paged one.  (Absent as above.)
    for cache in DECODE_CACHES:
        for fp8 in (False, True):
            append = append_entry_point(cache, fp8)
            if not hasattr(lib, append):
                continue
            getattr(lib, append).argtypes = ([vp, i64, i32, i32, i32, i32, i32, vp, vp, vp, vp]
                                             + ([vp, vp] if fp8 else [])
                                             + ([vp, i32, i32, i64] if cache == "paged" else []) + [vp, vp])
            getattr(lib, append).restype = ctypes.c_int
    lib.fa_estimate_forward_flops.argtypes = [P]
    lib.fa_estimate_forward_flops.restype = ctypes.c_double
    lib.fa_allowed_pairs.argtypes = [P]
    lib.fa_allowed_pairs.restype = ctypes.c_int64
    lib.fa_error_string.argtypes = [ctypes.c_int]
    lib.fa_error_string.restype = ctypes.c_char_p
    lib.fa_last_error.argtypes = []
    lib.fa_last_error.restype = ctypes.c_char_p
    lib.fa_rule_mask.argtypes = [P, vp]
    lib.fa_rule_mask.restype = ctypes.c_int
    lib.fa_rule_probe.argtypes = [P, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                  ctypes.POINTER(ctypes.c_int32)]
    lib.fa_rule_probe.restype = ctypes.c_int
    # (absent from a library built before the forward's choice function, as above)
    if hasattr(lib, "fa_forward_kernel"):
        lib.fa_forward_kernel.argtypes = [P, vp, vp, vp]
        lib.fa_forward_kernel.restype = ctypes.c_char_p
    lib.fa_build_info.argtypes = []
    lib.fa_build_info.restype = ctypes.c_char_p
    # the diagnostic library only (libfa_hip_diag.so): calls that reached a launch (0 forward, 1 backward), and
    # the slab launches of the batch-slab loops, which FA_SLAB_MAX shortens there (tests/test_gpu_slabs.py)
    if hasattr(lib, "fa_diag_call_count"):
        lib.fa_diag_call_count.argtypes = [ctypes.c_int]
        lib.fa_diag_call_count.restype = ctypes.c_longlong
    if hasattr(lib, "fa_diag_slab_count"):
        lib.fa_diag_slab_count.argtypes = []
        lib.fa_diag_slab_count.restype = ctypes.c_longlong
    return lib


def lib():
    """Load (once) and return the HIP library, or raise LibraryNotBuiltError."""
    global _lib
    ov = getattr(_tls, "override", None)
    if ov is not None:
        return ov
    if _process_override is not None:
        return _process_override
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise LibraryNotBuiltError(
                    f"HIP library not found at {LIB_PATH}; build it with "
                    "`python -c 'import __graft_entry__ as g; g.build()'` or `make -C tf_flash_attention_amd`")
            try:
                _lib = _declare(ctypes.CDLL(LIB_PATH))
            except OSError as e:  # pragma: no cover - environment problem
                raise LibraryNotBuiltError(f"failed to load {LIB_PATH}: {e}") from e
    return _lib


@contextlib.contextmanager
def using(path):
    """Route every call made inside the block through the library at ``path``.

    The GPU tests use it to run the diagnostic build (libfa_hip_diag.so, ``make -C
    tf_flash_attention_amd diag``): its FA_FWD_VARIANT / FA_BWD_VARIANT structures are not in
    the product library.  ctypes loads each library RTLD_LOCAL, so both can live in one process.
    The routing covers this thread and, while the block runs, every other thread of the process
    (autograd's device thread runs the backward of a CUDA tensor); blocks do not nest across
    threads: a second thread entering ``using()`` while another thread's block is open raises."""
    global _process_override, _process_owner, _process_depth
    me = threading.get_ident()
    with _lock:
        if _process_owner is not None and _process_owner != me:
            raise RuntimeError("_lib.using(): another thread's library override is active; "
                               "blocks may not overlap across threads")
        h = _loaded.get(path)
        if h is None:
            if not os.path.exists(path):
                raise LibraryNotBuiltError(f"library not found at {path}")
            h = _loaded[path] = _declare(ctypes.CDLL(path))
        prev = getattr(_tls, "override", None)
        prev_proc = _process_override
        _tls.override = h
        _process_override = h
        _process_owner = me
        _process_depth += 1
    try:
        yield h
    finally:
        with _lock:
            _tls.override = prev
            _process_override = prev_proc
            _process_depth -= 1
            if _process_depth == 0:
                _process_owner = None


def make_problem(dtype, policy, seq_dims, sync_mode, b, q_seq, k_seq, d, v_d,
                 window_size=1, log2_stride_size=0, is_causal=False) -> FaProblem:
    p = FaProblem()
    p.dtype, p.policy, p.seq_dims, p.sync_mode = dtype, policy, seq_dims, sync_mode
    p.b = int(b)
    for i in range(2):
        p.q_seq[i] = int(q_seq[i]) if i < len(q_seq) else 1
        p.k_seq[i] = int(k_seq[i]) if i < len(k_seq) else 1
    p.d, p.v_d = int(d), int(v_d)
    p.window_size, p.log2_stride_size, p.is_causal = int(window_size), int(log2_stride_size), int(bool(is_causal))
    return p


def pointer_array(ptrs):
    """A host array of device pointers (``const void* const*``) for fa_merge_partials / fa_accumulate_parts,
    or None (a null array) for ``ptrs`` None."""
    if ptrs is None:
        return None
    return (ctypes.c_void_p * len(ptrs))(*[int(p) if p else None for p in ptrs])


def source_hash(diag: bool = False) -> str:
    """sha256 (first 16 hex digits) of the product sources, computed exactly as the Makefile's
    SRC_HASH (csrc/*.hip, csrc/*.h, ../include/fa_api.h in make's byte-wise sort order); with
    ``diag`` the diagnostic library's DIAG_HASH, which also covers csrc/diag/*.hip."""
    import glob
    import hashlib
    files = glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h"))
    if diag:
        files += glob.glob(os.path.join(_HERE, "csrc", "diag", "*.hip"))
    rel = [os.path.relpath(p, _HERE) for p in files] + ["../include/fa_api.h"]
    h = hashlib.sha256()
    for r in sorted(rel, key=lambda x: x.encode()):
        with open(os.path.join(_HERE, r), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def build_info() -> str:
    return lib().fa_build_info().decode()


def last_error() -> str:
    return lib().fa_last_error().decode()
