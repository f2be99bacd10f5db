"""htm_hashjoin_amd -- MI355X-native hash-join build+probe engine.

Python is only a thin host layer over the C ABI of libhtmjoin_hip.so
(include/htm_hashjoin.h): the operators below mirror the free functions of the
reference (anilshanbhag/HTM-HashJoin) by name and argument meaning.
"""
from ._lib import (  # noqa: F401
    HJ_OK, HJ_ERR_INVALID, HJ_ERR_NO_DEVICE, HJ_ERR_HIP, HJ_ERR_OOM, HJ_ERR_KEY_RANGE,
    HJ_ERR_UNKNOWN_ALGO, HJ_ERR_STATE, HJ_FLAG_KEEP_ROW_IDS, HJ_FLAG_TRACK_R_MATCHES, HJ_FLAG_SLOT_CODES, HJ_R_UNMATCHED, HJ_R_MATCHED, LIB_PATH, hj_params, hj_result, lib,
    HJ_JOIN_INNER, HJ_JOIN_LEFT, HJ_JOIN_SEMI, HJ_JOIN_ANTI, HJ_NO_ROW, HJ_GATHER_MAX_COLS, hj_gather_col,
    HJ_KEY_MAX_COLS, HJ_KEY_SIDE_S, HJ_KEY_SIDE_R, hj_key_col, HJ_KEY_NULLS_EQUAL, hj_key_col2, hj_gather_col2,
    HJ_WHERE_MAX_TERMS, HJ_CMP_EQ, HJ_CMP_NE, HJ_CMP_LT, HJ_CMP_LE, HJ_CMP_GT, HJ_CMP_GE, CMP_OPS, HJ_VAL_UINT, HJ_VAL_INT, HJ_VAL_FLOAT,
    hj_where_term, ASOF_OPS, hj_asof_term,
    HJ_SORT_MAX_COLS, HJ_SORT_DESC, HJ_SORT_NULLS_FIRST, hj_sort_col,
    HJ_WIN_MAX_FUNCS, hj_win_func, HJ_FRAME_MAX_FUNCS, HJ_FRAME_UNBOUNDED_LO, HJ_FRAME_UNBOUNDED_HI, hj_frame_func,
    HJ_RANGE_LO_OPEN, HJ_RANGE_HI_OPEN, HJ_RANGE_ALL, HJ_RANGE_FIRST, HJ_RANGE_LAST, RANGE_PICKS, hj_range_term,
    HJ_AGG_MAX_COLS, HJ_AGG_COUNT, HJ_AGG_SUM, HJ_AGG_MIN, HJ_AGG_MAX, HJ_AGG_SIGNED, hj_agg_spec, hj_agg_src, hj_agg_col,
)
from .engine import (  # noqa: F401
    HashJoinError, HashJoinContext, NoCCHashBuild, AtomicHashBuild, HTMHashBuild, PRO, prj_agg_layout_info,
    generate_data, generate_relation, device_count, window_layout_info, frames_layout_info, wave_layout_info, htm_chain_layout_info, own_layout_info, slot_codes_info, ring_word_info, SHARD_ONE_BASED, BUCKET_DTYPE, NO_ROW,
)
from .columns import KeyColumn, key_hash_host, key_hash2_host  # noqa: F401
from .conditions import pairs_where_host, pairs_asof_host  # noqa: F401
from .joins import join_pairs, radix_join_pairs, outer_join_pairs, radix_outer_join_pairs, join_tables  # noqa: F401
from .key_joins import join_on, join_on_columns  # noqa: F401
from .aggregates import radix_join_aggregate, aggregate_on  # noqa: F401
from .groups import key_groups, key_groups_host, distinct_on, group_by_columns  # noqa: F401
from .sorting import sort_rows, sort_rows_host, sort_by_columns, sort_pairs  # noqa: F401
from .windows import window_rows, window_rows_host  # noqa: F401
from .ranges import range_join, interval_join, range_join_host, range_pairs_host, range_layout_info  # noqa: F401
