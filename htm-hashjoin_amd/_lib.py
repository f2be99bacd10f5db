"""ctypes binding of libhtmjoin_hip.so (C ABI: include/htm_hashjoin.h).

The library is the product; this module only declares its signatures. If the
shared object has not been built the import fails loudly -- there is no Python
or CPU fallback for any operator.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libhtmjoin_hip.so")

HJ_OK = 0
HJ_ERR_INVALID = -1
HJ_ERR_NO_DEVICE = -2
HJ_ERR_HIP = -3
HJ_ERR_OOM = -4
HJ_ERR_KEY_RANGE = -5
HJ_ERR_UNKNOWN_ALGO = -6
HJ_ERR_STATE = -7

HJ_ALGO_NOCC, HJ_ALGO_ATOMIC, HJ_ALGO_HTM, HJ_ALGO_PRJ, HJ_ALGO_AUTO = 0, 1, 2, 3, 4
ALGO_IDS = {"nocc": HJ_ALGO_NOCC, "atomic": HJ_ALGO_ATOMIC, "htm": HJ_ALGO_HTM, "prj": HJ_ALGO_PRJ,
            "auto": HJ_ALGO_AUTO}
ALGO_NAMES = {v: k for k, v in ALGO_IDS.items()}

# hj_params.flags: open addressing never leaves the table in the compact 4-byte format; the resident radix join keeps R
# as {key, row} elements (hj_prj_probe_pairs_dev)
HJ_FLAG_KEEP_ROW_IDS = 0x1
# hj_params.flags: the context keeps one bit per R row, set by every INNER / LEFT materialising probe for the R rows of the
# rows it produces (hj_r_rows_dev turns the bits into rows); needs HJ_FLAG_KEEP_ROW_IDS except on "htm"
HJ_FLAG_TRACK_R_MATCHES = 0x2
# hj_params.flags: the classic rings leave one code byte per slot (table format 2) whatever the table's size; without it
# only where a byte holds any 32-bit key (hj_slot_codes_info). For tests of the format at small sizes
HJ_FLAG_SLOT_CODES = 0x4
# hj_r_rows_dev: which rows
HJ_R_UNMATCHED, HJ_R_MATCHED = 0, 1

# hj_join_kind (hj_probe_join_dev / hj_prj_probe_join_dev) and the R row of a left-outer row without a match
HJ_JOIN_INNER, HJ_JOIN_LEFT, HJ_JOIN_SEMI, HJ_JOIN_ANTI = 0, 1, 2, 3
JOIN_KINDS = {"inner": HJ_JOIN_INNER, "left": HJ_JOIN_LEFT, "semi": HJ_JOIN_SEMI, "anti": HJ_JOIN_ANTI}
HJ_NO_ROW = 0xFFFFFFFF
# hj_gather_dev: columns of one call
HJ_GATHER_MAX_COLS = 8
# hj_key_hash_dev / hj_pairs_verify_dev: key columns of one call, and which side's pointers the hash reads
HJ_KEY_MAX_COLS = 4
HJ_KEY_SIDE_S, HJ_KEY_SIDE_R = 0, 1
# hj_key_col2.flags: in this column a NULL equals a NULL
HJ_KEY_NULLS_EQUAL = 0x1
# hj_pairs_where_dev: terms of one call, the comparison of a term (hj_cmp_op) and how its elements are read (hj_val_type)
HJ_WHERE_MAX_TERMS = 4
HJ_CMP_EQ, HJ_CMP_NE, HJ_CMP_LT, HJ_CMP_LE, HJ_CMP_GT, HJ_CMP_GE = 0, 1, 2, 3, 4, 5
CMP_OPS = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}
HJ_VAL_UINT, HJ_VAL_INT, HJ_VAL_FLOAT = 0, 1, 2
# hj_pairs_asof_dev: the ops that order (backward: >=, >; forward: <=, <)
ASOF_OPS = {op: CMP_OPS[op] for op in (">=", ">", "<=", "<")}
# hj_sort_rows_dev: columns of one call, and hj_sort_col.flags
HJ_SORT_MAX_COLS = 4
HJ_SORT_DESC, HJ_SORT_NULLS_FIRST = 0x1, 0x2
# hj_range_pairs_dev: hj_range_term.flags and hj_range_pick
HJ_RANGE_LO_OPEN, HJ_RANGE_HI_OPEN = 0x1, 0x2
HJ_RANGE_ALL, HJ_RANGE_FIRST, HJ_RANGE_LAST = 0, 1, 2
RANGE_PICKS = {"all": HJ_RANGE_ALL, "first": HJ_RANGE_FIRST, "last": HJ_RANGE_LAST}
# hj_window_rows_dev: functions of one call, and hj_win_op
HJ_WIN_MAX_FUNCS = 8
(HJ_WIN_ROW_NUMBER, HJ_WIN_RANK, HJ_WIN_DENSE_RANK, HJ_WIN_PART_ROWS, HJ_WIN_LAG, HJ_WIN_LEAD, HJ_WIN_FIRST_ROW, HJ_WIN_LAST_ROW,
 HJ_WIN_RUN_COUNT, HJ_WIN_RUN_SUM, HJ_WIN_RUN_MIN, HJ_WIN_RUN_MAX) = range(12)
# hj_window_frames_dev: functions of one call, and the frame bits of hj_frame_func.flags (beside HJ_AGG_SIGNED)
HJ_FRAME_MAX_FUNCS = 8
HJ_FRAME_UNBOUNDED_LO, HJ_FRAME_UNBOUNDED_HI = 0x2, 0x4
# aggregating joins (hj_agg_op, hj_agg_spec.flags)
HJ_AGG_MAX_COLS = 4
HJ_AGG_COUNT, HJ_AGG_SUM, HJ_AGG_MIN, HJ_AGG_MAX = 0, 1, 2, 3
AGG_OPS = {"count": HJ_AGG_COUNT, "sum": HJ_AGG_SUM, "min": HJ_AGG_MIN, "max": HJ_AGG_MAX}
HJ_AGG_SIGNED = 0x1


class hj_params(C.Structure):
    _fields_ = [
        ("algo", C.c_uint32),
        ("scaleOutput", C.c_uint32),
        ("numPartitions", C.c_uint32),
        ("probeLength", C.c_uint32),
        ("transactionSize", C.c_uint32),
        ("radixBits", C.c_uint32),
        ("buildVariant", C.c_uint32),
        ("prjMode", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32 * 3),
    ]


class hj_result(C.Structure):
    _fields_ = (
        [(n, C.c_uint64) for n in (
            "rSize", "sSize", "tableSize", "conflicts", "totalMatches", "inputSum",
            "tableSumHalf", "tableSumFull", "conflictSum", "outputSum", "prjChecksum",
            "prjPartitions")]
        + [("radixBits", C.c_uint32), ("buildVariant", C.c_uint32)]
        + [(n, C.c_double) for n in (
            "clear_us", "build_us", "probe_us", "partition_us", "join_us", "total_us", "h2d_us")]
        + [("buildDeferred", C.c_uint64), ("buildPhaseA_us", C.c_double), ("algoUsed", C.c_uint32),
           ("prjPath", C.c_uint32), ("foreignTuples", C.c_uint64), ("prjScatterPass1R_us", C.c_double),
           ("htmBuckets", C.c_uint64), ("htmOverflowBuckets", C.c_uint64), ("htmOverflowSum", C.c_uint64),
           ("compactFallback", C.c_uint64)]
    )

    def as_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("reserved")}
        d["algoUsed"] = ALGO_NAMES.get(d["algoUsed"], d["algoUsed"])
        return d


class hj_gather_col(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("width", C.c_uint32),
        ("reserved", C.c_uint32),
        ("fill", C.c_uint64 * 2),
    ]


class hj_gather_col2(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("dst", C.c_void_p),
        ("srcOffsets", C.c_void_p),
        ("dstOffsets", C.c_void_p),
        ("srcValid", C.c_void_p),
        ("dstValid", C.c_void_p),
        ("dstCapacity", C.c_uint64),
        ("width", C.c_uint32),
        ("flags", C.c_uint32),
        ("fill", C.c_uint64 * 2),
    ]


class hj_key_col(C.Structure):
    _fields_ = [
        ("s", C.c_void_p),
        ("r", C.c_void_p),
        ("width", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class hj_key_col2(C.Structure):
    _fields_ = [
        ("s", C.c_void_p),
        ("r", C.c_void_p),
        ("sOffsets", C.c_void_p),
        ("rOffsets", C.c_void_p),
        ("sValid", C.c_void_p),
        ("rValid", C.c_void_p),
        ("width", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class hj_where_term(C.Structure):
    _fields_ = [
        ("s", C.c_void_p),
        ("r", C.c_void_p),
        ("sValid", C.c_void_p),
        ("rValid", C.c_void_p),
        ("width", C.c_uint32),
        ("type", C.c_uint32),
        ("op", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class hj_asof_term(C.Structure):
    _fields_ = list(hj_where_term._fields_)     # the same layout; op is one of GE, GT, LE, LT


class hj_sort_col(C.Structure):
    _fields_ = [
        ("values", C.c_void_p),
        ("valid", C.c_void_p),
        ("width", C.c_uint32),
        ("type", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class hj_range_term(C.Structure):
    _fields_ = [
        ("lo", C.c_void_p),
        ("hi", C.c_void_p),
        ("loValid", C.c_void_p),
        ("hiValid", C.c_void_p),
        ("width", C.c_uint32),
        ("type", C.c_uint32),
        ("flags", C.c_uint32),
        ("pick", C.c_uint32),
    ]


class hj_frame_func(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("srcValid", C.c_void_p),
        ("out", C.c_void_p),
        ("lo", C.c_int64),
        ("hi", C.c_int64),
        ("op", C.c_uint32),
        ("width", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class hj_win_func(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("srcValid", C.c_void_p),
        ("out", C.c_void_p),
        ("op", C.c_uint32),
        ("width", C.c_uint32),
        ("flags", C.c_uint32),
        ("offset", C.c_uint32),
    ]


class hj_agg_spec(C.Structure):
    _fields_ = [
        ("op", C.c_uint32),
        ("width", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class hj_agg_src(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("srcValid", C.c_void_p),
    ]


class hj_agg_col(C.Structure):
    _fields_ = [
        ("src", C.c_void_p),
        ("srcValid", C.c_void_p),
        ("acc", C.c_void_p),
        ("op", C.c_uint32),
        ("width", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


def _declare(lib):
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    P = C.POINTER
    sig = {
        "hj_abi_version": ([], i32),
        "hj_device_count": ([P(i32)], i32),
        "hj_create": ([i32, P(vp)], i32),
        "hj_create_on_stream": ([i32, vp, P(vp)], i32),
        "hj_destroy": ([vp], None),
        "hj_strerror": ([i32], C.c_char_p),
        "hj_last_error": ([vp], C.c_char_p),
        "hj_synchronize": ([vp], i32),
        "hj_run": ([vp, P(hj_params), vp, u64, vp, u64, P(hj_result)], i32),
        "hj_reserve": ([vp, P(hj_params), u64, u64], i32),
        "hj_build_dev": ([vp, vp, u64, u64], i32),
        "hj_probe_dev": ([vp, vp, u64], i32),
        "hj_probe_pairs_dev": ([vp, vp, u64, u64, vp, vp, u64], i32),
        "hj_probe_join_dev": ([vp, u32, vp, u64, u64, vp, vp, u64], i32),
        "hj_pairs_info": ([vp, P(u64)], i32),
        "hj_r_marks_clear": ([vp], i32),
        "hj_r_rows_dev": ([vp, u32, vp, u64], i32),
        "hj_r_rows_info": ([vp, P(u64)], i32),
        "hj_gather_dev": ([vp, vp, u64, u32, u64, P(hj_gather_col), u32, vp], i32),
        "hj_gather_info": ([vp, P(u64)], i32),
        "hj_gather2_dev": ([vp, vp, u64, u32, u64, P(hj_gather_col2), u32, vp], i32),
        "hj_gather2_info": ([vp, P(u64)], i32),
        "hj_key_hash_dev": ([vp, P(hj_key_col), u32, u32, u64, u32, vp], i32),
        "hj_key_hash_host": ([P(hj_key_col), u32, u32, u64, u32, vp], i32),
        "hj_pairs_verify_dev": ([vp, vp, vp, u64, u32, u64, u64, P(hj_key_col), u32, vp, vp, u64, vp, vp], i32),
        "hj_verify_info": ([vp, P(u64)], i32),
        "hj_key_hash2_dev": ([vp, P(hj_key_col2), u32, u32, u64, u32, vp], i32),
        "hj_key_hash2_host": ([P(hj_key_col2), u32, u32, u64, u32, vp], i32),
        "hj_pairs_verify2_dev": ([vp, vp, vp, u64, u32, u64, u64, P(hj_key_col2), u32, vp, vp, u64, vp, vp], i32),
        "hj_key_groups_dev": ([vp, P(hj_key_col2), u32, u32, u64, u32, vp, vp, vp, u64], i32),
        "hj_key_groups_info": ([vp, P(u64)], i32),
        "hj_key_groups_host": ([P(hj_key_col2), u32, u32, u64, u32, vp, vp, vp, u64, P(u64)], i32),
        "hj_sort_rows_dev": ([vp, P(hj_sort_col), u32, u64, vp], i32),
        "hj_sort_rows_info": ([vp, P(u64)], i32),
        "hj_sort_rows_host": ([P(hj_sort_col), u32, u64, vp, P(u64)], i32),
        "hj_sort_layout_info": ([u64, P(u64)], i32),
        "hj_window_rows_dev": ([vp, vp, u64, u64, vp, P(hj_sort_col), u32, P(hj_win_func), u32], i32),
        "hj_window_rows_info": ([vp, P(u64)], i32),
        "hj_window_rows_host": ([vp, u64, u64, vp, P(hj_sort_col), u32, P(hj_win_func), u32, P(u64)], i32),
        "hj_window_layout_info": ([u64, P(u64)], i32),
        "hj_window_frames_dev": ([vp, vp, u64, u64, vp, P(hj_frame_func), u32], i32),
        "hj_window_frames_info": ([vp, P(u64)], i32),
        "hj_window_frames_host": ([vp, u64, u64, vp, P(hj_frame_func), u32, P(u64)], i32),
        "hj_frames_layout_info": ([u64, P(u64)], i32),
        "hj_range_index_dev": ([vp, P(hj_sort_col), u64, vp, vp, vp], i32),
        "hj_range_index_info": ([vp, P(u64)], i32),
        "hj_range_index_host": ([P(hj_sort_col), u64, vp, vp, vp], i32),
        "hj_range_layout_info": ([u64, u64, P(u64)], i32),
        "hj_range_pairs_dev": ([vp, vp, vp, vp, u64, P(hj_range_term), u64, u32, vp, vp, u64, vp, vp], i32),
        "hj_range_pairs_info": ([vp, P(u64)], i32),
        "hj_range_pairs_host": ([vp, vp, vp, u64, P(hj_range_term), u64, u32, vp, vp, u64, vp, vp, P(u64)], i32),
        "hj_pairs_where_dev": ([vp, vp, vp, u64, u32, u64, u64, P(hj_where_term), u32, vp, vp, u64, vp, vp], i32),
        "hj_where_info": ([vp, P(u64)], i32),
        "hj_pairs_where_host": ([vp, vp, u64, u32, u64, u64, P(hj_where_term), u32, vp, vp, u64, vp, vp, P(u64)], i32),
        "hj_pairs_asof_dev": ([vp, vp, vp, u64, u32, u64, u64, P(hj_asof_term), vp, vp, vp, vp, u64, vp, vp], i32),
        "hj_asof_info": ([vp, P(u64)], i32),
        "hj_pairs_asof_host": ([vp, vp, u64, u32, u64, u64, P(hj_asof_term), vp, vp, vp, vp, u64, vp, vp, P(u64)], i32),
        "hj_mark_rows_dev": ([vp, vp, u64, u32, u32, vp, u64], i32),
        "hj_mark_rows_info": ([vp, P(u64)], i32),
        "hj_prj_join_dev": ([vp, vp, u64, vp, u64], i32),
        "hj_prj_build_dev": ([vp, vp, u64], i32),
        "hj_prj_probe_dev": ([vp, vp, u64], i32),
        "hj_prj_probe_pairs_dev": ([vp, vp, u64, u64, vp, vp, u64], i32),
        "hj_prj_probe_join_dev": ([vp, u32, vp, u64, u64, vp, vp, u64], i32),
        "hj_prj_resident_info": ([vp, P(u64)], i32),
        "hj_prj_agg_begin": ([vp, P(hj_agg_spec), u32], i32),
        "hj_prj_probe_agg_dev": ([vp, vp, u64, P(hj_agg_src), u32], i32),
        "hj_prj_agg_rows_dev": ([vp, P(vp), vp], i32),
        "hj_prj_agg_info": ([vp, P(u64)], i32),
        "hj_prj_agg_layout_info": ([u32, P(u64)], i32),
        "hj_pairs_agg_dev": ([vp, vp, vp, u64, u32, u64, u32, u64, P(hj_agg_col), u32, vp], i32),
        "hj_pairs_agg_info": ([vp, P(u64)], i32),
        "hj_join_dev": ([vp, vp, u64, vp, u64], i32),
        "hj_checksums_dev": ([vp], i32),
        "hj_fetch_result": ([vp, P(hj_result)], i32),
        "hj_export_table": ([vp, vp, u64], i32),
        "hj_export_buckets": ([vp, vp, u64, vp, u64, P(u64)], i32),
        "hj_shard_histogram_dev": ([vp, vp, u64, u32, u32, vp], i32),
        "hj_shard_scatter_dev": ([vp, vp, u64, u32, u32, vp, vp], i32),
        "hj_build_keys_dev": ([vp, vp, u64, u32, u64], i32),
        "hj_probe_keys_dev": ([vp, vp, u64], i32),
        "hj_set_shard_check": ([vp, u32, u32, u32], i32),
        "hj_dev_alloc": ([vp, u64, P(vp)], i32),
        "hj_dev_free": ([vp, vp], i32),
        "hj_copy_h2d": ([vp, vp, vp, u64], i32),
        "hj_copy_d2h": ([vp, vp, vp, u64], i32),
        "hj_prj_workspace_info": ([u64, u64, u32, P(u64)], i32),
        "hj_prj_fragment_info": ([u64, u64, u32, u32, P(u64)], i32),
        "hj_wave_layout_info": ([vp, u32, u64, P(u64)], i32),
        "hj_wave_seams": ([vp, vp, vp, vp, u64, P(u64)], i32),
        "hj_wave_planar_info": ([vp, P(u64)], i32),
        "hj_slot_codes_info": ([vp, u64, u32, P(u64)], i32),
        "hj_ring_word_layout_info": ([u64, u32, u32, u32, u32, P(u64)], i32),
        "hj_table_debug": ([vp, P(u64)], i32),
        "hj_htm_chain_layout_info": ([vp, u32, u64, P(u64)], i32),
        "hj_htm_chain_info": ([vp, P(u64)], i32),
        "hj_own_layout_info": ([vp, u32, u64, P(u64)], i32),
        "hj_own_info": ([vp, vp, u64, vp, u64, P(u64)], i32),
        "hj_zipf_open": ([vp, u64, C.c_double, C.c_uint], i32),
        "hj_zipf_next_dev": ([vp, u64, vp], i32),
        "hj_zipf_close": ([vp], i32),
        "hj_generate_relation": ([C.c_char_p, u64, u64, i32, C.c_double, C.c_uint, vp], i32),
        "hj_generate_data": ([C.c_char_p, u64, u64, i32, C.c_double, vp], i32),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.argtypes = args
        fn.restype = res
    return sig


def load():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C htm-hashjoin_amd/csrc`. There is no fallback implementation."
        )
    lib = C.CDLL(LIB_PATH)
    lib._hj_signatures = _declare(lib)
    return lib


lib = load()
