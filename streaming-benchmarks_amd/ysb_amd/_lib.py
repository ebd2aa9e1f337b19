"""ctypes binding of libysb_hip.so (include/ysb_hip.h).

The library is built in-tree (streaming-benchmarks_amd/lib/libysb_hip.so) by
`make -C streaming-benchmarks_amd` / __graft_entry__.build().  There is no CPU
fallback: if the library is missing, importing a compute entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# YSB_LIB_VARIANT=stamps selects the diagnostic build (tools/stamps.py only)
LIB_PATH = os.path.join(PKG_ROOT, "lib", "libysb_hip%s.so" % (
    "_" + os.environ["YSB_LIB_VARIANT"] if os.environ.get("YSB_LIB_VARIANT") else ""))

YSB_OK = 0
YSB_PENDING = 1
ERRORS = {-1: "YSB_ERR_ARG", -2: "YSB_ERR_HIP", -3: "YSB_ERR_STATE", -4: "YSB_ERR_CAPACITY",
          -5: "YSB_ERR_FORMAT", -6: "YSB_ERR_RCCL", -7: "YSB_ERR_NOMEM", -8: "YSB_ERR_DATA"}

YSB_F_TIMING = 0x1
YSB_F_REQUIRE_IP = 0x2
YSB_F_NO_LDS_COUNT = 0x4
YSB_F_SPARSE_FAST_JOIN = 0x8
YSB_F_FORMAT_TBL = 0x10
YSB_F_RECORD_COUNT = 0x20
YSB_F_NO_RECORD_COUNT = 0x40
YSB_F_COMPACT_FIRST = 0x80
YSB_F_FLAT_FIRST = 0x100
YSB_F_LAYOUT_AUTO = 0x200   # the default since ABI 2 (accepted, ignored)
YSB_F_STRICT = 0x400
YSB_F_LAYOUT_FIXED = 0x800
YSB_F_H2D_SDMA = 0x1000
YSB_SUM_TRUTH_BLOCKS = 0
YSB_SUM_PENDING_BLOCKS = 1
YSB_SUM_OWNED = 2
INT64_MIN = -(1 << 63)
UNIQUE_ID_BYTES = 128


class YsbConfig(C.Structure):
    _fields_ = [("time_divisor_ms", C.c_int64), ("n_campaigns", C.c_uint32), ("window_ring", C.c_uint32),
                ("max_ads", C.c_uint64), ("max_batch_events", C.c_uint64), ("max_batch_bytes", C.c_uint64),
                ("ring_base_bucket", C.c_int64), ("overflow_capacity", C.c_uint64), ("flags", C.c_uint32),
                ("reserved", C.c_uint32)]


class YsbStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("events", "views", "joined", "join_misses", "parse_errors",
                                          "time_errors", "out_of_ring", "overflow_dropped", "batches", "deferred",
                                          "foreign_shard")]


class YsbCount(C.Structure):
    _fields_ = [("campaign", C.c_uint32), ("reserved", C.c_uint32), ("window_ms", C.c_int64),
                ("count", C.c_uint64)]


class YsbExchangeInfo(C.Structure):
    _fields_ = [("exchanges", C.c_uint64), ("bytes", C.c_uint64), ("ms", C.c_double), ("last_buckets", C.c_uint32),
                ("last_width", C.c_uint32), ("full_ring_bytes", C.c_uint64), ("critical_ms", C.c_double),
                ("rs_ms", C.c_double), ("exposed_ms", C.c_double)]


class YsbRebase(C.Structure):
    _fields_ = [("first_line", C.c_uint64), ("lead_shift", C.c_int64)]


class YsbLaunchDesc(C.Structure):
    _fields_ = [("layout", C.c_uint32), ("record_mode", C.c_uint32), ("hbm_table", C.c_uint32), ("tbl", C.c_uint32)]


class YsbRecordDesc(C.Structure):
    _fields_ = [("w_log2", C.c_uint32), ("blk_shift", C.c_uint32), ("n_blocks", C.c_uint32), ("sub_log2", C.c_uint32),
                ("bins", C.c_uint32), ("cap", C.c_uint32), ("grid", C.c_uint32), ("slices", C.c_uint32),
                ("area", C.c_uint64), ("part", C.c_uint64), ("delta_bound", C.c_uint64), ("dirty", C.c_uint32),
                ("reserved", C.c_uint32)]


ALLREDUCE_MAX_FN =C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64)
REDUCE_SCATTER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32)


class YsbCollectives(C.Structure):
    _fields_ = [("allreduce_max_u64", ALLREDUCE_MAX_FN), ("reduce_scatter_sum", REDUCE_SCATTER_FN),
                ("user", C.c_void_p)]


class YsbSegment(C.Structure):
    _fields_ = [("d_bytes", C.c_void_p), ("nbytes", C.c_uint64), ("d_line_off", C.c_void_p),
                ("n_events", C.c_uint64)]


YSB_COL_JAVA_ORDER = 0x1
YSB_COL_VALIDITY = 0x2


class YsbColumnsLayout(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("start", C.c_uint64 * 9), ("width", C.c_uint32 * 7),
                ("reserved", C.c_uint32), ("image_bytes", C.c_uint64)]


class YsbDecodeInfo(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("valid", C.c_uint64), ("fast_rows", C.c_uint64),
                ("kernel_ms", C.c_double)]


class YsbColcountDesc(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("lds_counters", C.c_uint32), ("hbm_table", C.c_uint32),
                ("java_order", C.c_uint32), ("validity", C.c_uint32)]


YSB_JOIN_KEYS = 0x1


class YsbJoinedLayout(C.Structure):
    _fields_ = [("cap_rows", C.c_uint64), ("start", C.c_uint64 * 7), ("width", C.c_uint32 * 6),
                ("flags", C.c_uint32), ("n_cols", C.c_uint32)]


class YsbJoinInfo(C.Structure):
    _fields_ = ([(n, C.c_uint64) for n in ("events", "views", "joined", "join_misses", "parse_errors", "time_errors",
                                           "foreign_shard", "rows_written", "fast_rows", "tiles")]
                + [("grid", C.c_uint32), ("max_grid", C.c_uint32)]
                + [(n, C.c_double) for n in ("join_ms", "prefix_ms", "pack_ms")])


class YsbUpsertInfo(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("entries", "foreign", "duplicates", "updated", "inserted", "cuckoo_first",
                                          "cuckoo_second", "cuckoo_moved", "cuckoo_left_out")] + [
                ("rebuilt", C.c_uint32), ("partial", C.c_uint32), ("device_ms", C.c_double)]


class YsbAdmapDesc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("keys", "keys36", "table_slots", "ctable_slots")] + [
                (n, C.c_uint32) for n in ("buckets", "partial", "shard_rank", "shard_n")]


class YsbParkedDesc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("capacity", "parked", "parked_total", "dropped", "resolved_joined",
                                          "resolved_missed", "resolved_time_errors", "distinct_keys")] + [
                ("distinct_ms", C.c_double), ("resolve_ms", C.c_double)]


class YsbLz4Block(C.Structure):
    _fields_ = [("comp_bytes", C.c_uint32), ("raw_bytes", C.c_uint32)]


class YsbLz4Desc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("batches", "blocks", "stored_blocks", "comp_bytes", "raw_bytes",
                                          "bad_blocks", "first_bad")] + [("decode_ms", C.c_double)]


class YsbLz4FrameBlock(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("comp_bytes", C.c_uint32), ("reserved", C.c_uint32)]


class YsbLz4FrameSummary(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("frames", "skippable_frames", "blocks", "stored_blocks", "comp_bytes",
                                          "content_bytes")] + [
                (n, C.c_uint32) for n in ("block_checksums", "content_checksums", "content_sizes", "reserved")]


class YsbLz4FrameDesc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("blocks", "stored_blocks", "comp_bytes", "raw_bytes", "bad_blocks",
                                          "first_bad", "decoder", "batches", "carry_in", "carry_out")] + [
                ("measure_ms", C.c_double), ("decode_ms", C.c_double)]


class YsbKafkaBatch(C.Structure):
    _fields_ = [("records_off", C.c_uint64), ("records_bytes", C.c_uint32), ("n_records", C.c_uint32),
                ("first_record", C.c_uint64), ("base_offset", C.c_int64), ("control_before", C.c_uint32),
                ("reserved", C.c_uint32)]


class YsbKafkaSummary(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_batches", "n_records", "consumed", "control_batches", "crc_checked")]


class YsbKafkaVerdict(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("bad_batches", "first_bad", "record", "rule")]


class YsbKafkaCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("records", "null_values", "keyed", "headers", "value_bytes")]


class YsbKafkaPackOpts(C.Structure):
    _fields_ = [("batch_bytes", C.c_uint32), ("batch_records", C.c_uint32), ("base_offset", C.c_int64),
                ("base_timestamp", C.c_int64), ("key_off", C.c_void_p), ("keys", C.c_void_p), ("ts_delta", C.c_void_p),
                ("n_headers", C.c_uint32), ("codec", C.c_uint32), ("header_keys", C.POINTER(C.c_char_p)),
                ("header_vals", C.POINTER(C.c_char_p)), ("header_val_len", C.POINTER(C.c_int32)),
                ("snappy_framing", C.c_uint32), ("snappy_chunk", C.c_uint32)]


class YsbKafkaDesc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("calls", "batches", "records", "null_values", "keyed", "headers",
                                          "control_skipped", "framed_bytes", "value_bytes", "window_bytes")] + [
                ("verdict", YsbKafkaVerdict), ("walk_ms", C.c_double), ("base_ms", C.c_double), ("gather_ms", C.c_double)]


class YsbKafkaCrcDesc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("calls", "mode", "batches", "bytes", "bad_batches", "first_bad")] + [
                ("stored", C.c_uint32), ("computed", C.c_uint32), ("grid_waves", C.c_uint64), ("crc_ms", C.c_double)]


class YsbKafkaFrame(C.Structure):
    _fields_ = [("first_block", C.c_uint64), ("n_blocks", C.c_uint32), ("codec", C.c_uint32)]


class YsbKafkaLz4Summary(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_batches", "n_records", "consumed", "control_batches", "crc_checked",
                                          "compressed_batches", "blocks", "stored_blocks", "comp_bytes")]


class YsbKafkaLz4Desc(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("calls", "blocks", "stored_blocks", "compressed_batches", "wire_bytes",
                                          "inflated_bytes", "bad_blocks", "decoder", "inflated_buffer_bytes",
                                          "inflated_total")] + [
                ("measure_ms", C.c_double), ("plan_ms", C.c_double), ("decode_ms", C.c_double),
                ("snappy_blocks", C.c_uint64), ("preamble_ms", C.c_double)]


class YsbGenParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_campaigns", C.c_uint32), ("ads_per_campaign", C.c_uint32),
                ("t0_ms", C.c_int64), ("events_per_sec", C.c_uint64), ("with_skew", C.c_uint32),
                ("n_users", C.c_uint32), ("ad_subset", C.POINTER(C.c_uint32)), ("n_ad_subset", C.c_uint32),
                ("event_stream", C.c_uint32),
                ("format", C.c_uint32), ("variant", C.c_uint32)]


_P = C.c_void_p
_I = C.c_int
_U32 = C.c_uint32
_U64 = C.c_uint64
_I64 = C.c_int64
_PU8 = C.c_void_p
_PU32 = C.c_void_p

# name -> (restype, argtypes); every function include/ysb_hip.h declares.
SIGNATURES = {
    "ysb_abi_version": (_I, []),
    "ysb_device_count": (_I, []),
    "ysb_device_sync": (_I, [_I]),
    "ysb_device_numa_node": (_I, [_I]),
    "ysb_config_default": (None, [C.POINTER(YsbConfig)]),
    "ysb_open": (_I, [C.POINTER(_P), _I, C.POINTER(YsbConfig)]),
    "ysb_close": (_I, [_P]),
    "ysb_last_error": (C.c_char_p, [_P]),
    "ysb_load_ad_map": (_I, [_P, C.POINTER(C.c_char_p), C.POINTER(_U32), C.POINTER(_U32), _U64]),
    "ysb_load_ad_map_packed": (_I, [_P, C.c_void_p, _U32, C.c_void_p, _U64]),
    "ysb_load_ad_map_shard": (_I, [_P, C.POINTER(C.c_char_p), C.POINTER(_U32), C.POINTER(_U32), _U64, _U32, _U32]),
    "ysb_load_ad_map_packed_shard": (_I, [_P, C.c_void_p, _U32, C.c_void_p, _U64, _U32, _U32]),
    "ysb_ad_map_upsert": (_I, [_P, C.POINTER(C.c_char_p), C.POINTER(_U32), C.POINTER(_U32), _U64,
                               C.POINTER(YsbUpsertInfo)]),
    "ysb_ad_map_upsert_packed": (_I, [_P, C.c_void_p, _U32, C.c_void_p, _U64, C.POINTER(YsbUpsertInfo)]),
    "ysb_upsert_info_size": (_U64, []),
    "ysb_ad_map_lookup": (_I, [_P, C.POINTER(C.c_char_p), C.POINTER(_U32), _U64, _PU32, _PU32]),
    "ysb_ad_map_info": (_I, [_P, C.POINTER(YsbAdmapDesc)]),
    "ysb_admap_desc_size": (_U64, []),
    "ysb_parked_enable": (_I, [_P, _U64]),
    "ysb_parked_keys": (_I, [_P, C.c_void_p, _PU32, _U64, C.POINTER(_U64)]),
    "ysb_parked_resolve": (_I, [_P, C.POINTER(YsbParkedDesc)]),
    "ysb_parked_info": (_I, [_P, C.POINTER(YsbParkedDesc)]),
    "ysb_parked_info_size": (_U64, []),
    "ysb_slot_buffers": (_I, [_P, _I, C.POINTER(_P), C.POINTER(_P)]),
    "ysb_submit": (_I, [_P, _I, _PU8, _U64, _PU32, _U64]),
    "ysb_wait": (_I, [_P, _I]),
    "ysb_slot_capacity": (_I, [_P, C.POINTER(_U64), C.POINTER(_U64)]),
    "ysb_submit_raw": (_I, [_P, _I, _PU8, _U64]),
    "ysb_host_register": (_I, [_P, _P, _U64]),
    "ysb_host_unregister": (_I, [_P, _P]),
    "ysb_rebase_table": (_I, [_P, C.c_void_p, _U64, _I64]),
    "ysb_submit_raw_mapped": (_I, [_P, _I, _PU8, _U64, C.POINTER(YsbRebase)]),
    "ysb_submit_mapped": (_I, [_P, _I, _PU8, _U64, _PU32, _U64, C.POINTER(YsbRebase)]),
    "ysb_split_lines_device": (_I, [_P, _PU8, _U64, _PU32, _U64, C.POINTER(_U64)]),
    "ysb_submit_raw_lz4": (_I, [_P, _I, _PU8, _U64, _P, _U32]),
    "ysb_submit_lz4_mapped": (_I, [_P, _I, _PU8, _U64, _P, _U32, _PU32, _U64, C.POINTER(YsbRebase)]),
    "ysb_lz4_decode_device": (_I, [_P, _PU8, _U64, _P, _U32, _PU8, _U64, C.POINTER(_U64), C.POINTER(_U32)]),
    "ysb_lz4_info": (_I, [_P, C.POINTER(YsbLz4Desc)]),
    "ysb_lz4_desc_size": (_U64, []),
    "ysb_lz4_compress_bound": (_U32, [_U32]),
    "ysb_lz4_compress_block": (_I, [_PU8, _U32, _PU8, _U32, _I, C.POINTER(YsbLz4Block)]),
    "ysb_lz4_decompress_block": (_I, [_PU8, C.POINTER(YsbLz4Block), _PU8, _U32]),
    "ysb_lz4_write_file": (_I, [C.c_char_p, _PU8, _U64, _U32, _I, _I, _I]),
    "ysb_lz4_frame_index": (_I, [_PU8, _U64, _P, _U64, C.POINTER(_U64), C.POINTER(YsbLz4FrameSummary)]),
    "ysb_lz4_frame_bound": (_U64, [_U64, _U32]),
    "ysb_lz4_frame_pack": (_I, [_PU8, _U64, _U32, _I, _PU8, _U64, C.POINTER(_U64)]),
    "ysb_lz4_frame_write": (_I, [C.c_char_p, _PU8, _U64, _U32, _I]),
    "ysb_lz4_measure_block": (_I, [_PU8, _U32, C.POINTER(_U32)]),
    "ysb_lz4_frame_carry_cut": (_U64, [_PU8, _U64, _I]),
    "ysb_lz4_measure_device": (_I, [_P, _PU8, _P, _U32, _PU32, C.POINTER(_U32)]),
    "ysb_lz4_decode_blocks_device": (_I, [_P, _PU8, _P, _U32, _PU8, _U64, C.POINTER(_U64), C.POINTER(_U32)]),
    "ysb_submit_lz4_blocks": (_I, [_P, _I, _PU8, _P, _U32, _U32]),
    "ysb_submit_lz4_blocks_mapped": (_I, [_P, _I, _PU8, _P, _U32, _U32]),
    "ysb_lz4_set_decoder": (_I, [_P, _I]),
    "ysb_lz4_frame_info": (_I, [_P, C.POINTER(YsbLz4FrameDesc)]),
    "ysb_lz4_frame_desc_size": (_U64, []),
    "ysb_kafka_index": (_I, [_PU8, _U64, _U32, _P, _U64, C.POINTER(YsbKafkaSummary)]),
    "ysb_kafka_crc32c": (_U32, [_PU8, _U64]),
    "ysb_kafka_unframe_host": (_I, [_PU8, _U64, _P, _U64, _PU8, _U64, _PU32, _U64, C.POINTER(_U64), C.POINTER(_U64),
                                    C.POINTER(YsbKafkaCounters), C.POINTER(YsbKafkaVerdict)]),
    "ysb_kafka_bound": (_U64, [_U64, _U64, C.POINTER(YsbKafkaPackOpts)]),
    "ysb_kafka_pack": (_I, [_PU8, _U64, _PU32, _U64, C.POINTER(YsbKafkaPackOpts), _PU8, _U64, C.POINTER(_U64),
                            C.POINTER(_U64)]),
    "ysb_kafka_write_file": (_I, [C.c_char_p, _PU8, _U64, _PU32, _U64, C.POINTER(YsbKafkaPackOpts)]),
    "ysb_kafka_unframe_device": (_I, [_P, _PU8, _U64, _P, _U64, _PU8, _U64, _PU32, _U64, C.POINTER(_U64),
                                      C.POINTER(_U64)]),
    "ysb_submit_kafka": (_I, [_P, _I, _PU8, _U64, _P, _U64]),
    "ysb_submit_kafka_mapped": (_I, [_P, _I, _PU8, _U64, _P, _U64]),
    "ysb_kafka_info": (_I, [_P, C.POINTER(YsbKafkaDesc)]),
    "ysb_kafka_index_lz4": (_I, [_PU8, _U64, _U32, _P, _P, _U64, _P, _U64, C.POINTER(YsbKafkaLz4Summary)]),
    "ysb_kafka_unframe_lz4_host": (_I, [_PU8, _U64, _P, _P, _U64, _P, _U64, _PU8, _U64, _PU32, _U64, C.POINTER(_U64),
                                        C.POINTER(_U64), C.POINTER(_U64), C.POINTER(YsbKafkaCounters),
                                        C.POINTER(YsbKafkaVerdict)]),
    "ysb_kafka_unframe_lz4_device": (_I, [_P, _PU8, _U64, _P, _P, _U64, _P, _U64, _PU8, _U64, _PU32, _U64,
                                          C.POINTER(_U64), C.POINTER(_U64)]),
    "ysb_submit_kafka_lz4": (_I, [_P, _I, _PU8, _U64, _P, _P, _U64, _P, _U64]),
    "ysb_submit_kafka_lz4_mapped": (_I, [_P, _I, _PU8, _U64, _P, _P, _U64, _P, _U64]),
    "ysb_kafka_lz4_info": (_I, [_P, C.POINTER(YsbKafkaLz4Desc)]),
    "ysb_kafka_set_crc": (_I, [_P, _I]),
    "ysb_kafka_set_codecs": (_I, [_P, _U32]),
    "ysb_kafka_test_inflated_cap": (_I, [_P, _U64]),
    "ysb_kafka_inflate_bounds": (_I, [_PU8, _U64, _P, _P, _U64, _P, _U64, _P]),
    "ysb_snappy_compress_block": (_I, [_PU8, _U32, _PU8, _U32, C.POINTER(_U32)]),
    "ysb_snappy_decompress_block": (_I, [_PU8, _U32, _PU8, _U32, C.POINTER(_U32)]),
    "ysb_kafka_crc_device": (_I, [_P, _PU8, _U64, _P, _U64, _PU32, _PU32]),
    "ysb_kafka_crc_info": (_I, [_P, C.POINTER(YsbKafkaCrcDesc)]),
    "ysb_kafka_crc_desc_size": (_U64, []),
    "ysb_kafka_verdict_crc_host": (_I, [_PU8, _U64, _P, _U64, C.POINTER(YsbKafkaVerdict)]),
    "ysb_kafka_verdict_crc_lz4_host": (_I, [_PU8, _U64, _P, _P, _U64, _P, _U64, C.POINTER(YsbKafkaVerdict)]),
    "ysb_kafka_frame_size": (_U64, []),
    "ysb_kafka_lz4_summary_size": (_U64, []),
    "ysb_kafka_lz4_desc_size": (_U64, []),
    "ysb_kafka_batch_size": (_U64, []),
    "ysb_kafka_summary_size": (_U64, []),
    "ysb_kafka_verdict_size": (_U64, []),
    "ysb_kafka_counters_size": (_U64, []),
    "ysb_kafka_pack_opts_size": (_U64, []),
    "ysb_kafka_desc_size": (_U64, []),
    "ysb_lz4_pack": (_I, [_PU8, _U64, _U32, _I, _I, _I, _PU8, _U64, C.POINTER(_U64), _P, _U64, C.POINTER(_U64)]),
    "ysb_copy_time": (_I, [_P, C.POINTER(C.c_double), C.POINTER(_U64), C.POINTER(_U64)]),
    "ysb_submit_device": (_I, [_P, _PU8, _U64, _PU32, _U64]),
    "ysb_submit_device_segments": (_I, [_P, C.c_void_p, _U32]),
    "ysb_columns_layout_of": (_I, [_U64, C.POINTER(YsbColumnsLayout)]),
    "ysb_decode_columns_device": (_I, [_P, _PU8, _U64, _PU32, _U64, _PU8, _U64, _I64, _U32,
                                       C.POINTER(YsbDecodeInfo)]),
    "ysb_columns_read_ranges": (_I, [_U64, _U64, _U32, C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U32)]),
    "ysb_submit_columns_device": (_I, [_P, _PU8, _U64, _U64, _U32]),
    "ysb_submit_columns": (_I, [_P, _I, _PU8, _U64, _U64, _U32]),
    "ysb_columns_launch_info": (_I, [_P, C.POINTER(YsbColcountDesc)]),
    "ysb_colcount_desc_size": (_U64, []),
    "ysb_joined_layout_of": (_I, [_U64, _U32, C.POINTER(YsbJoinedLayout)]),
    "ysb_join_device": (_I, [_P, _PU8, _U64, _PU32, _U64, _PU8, _U64, _U32, C.POINTER(YsbJoinInfo)]),
    "ysb_join_info_size": (C.c_size_t, []),
    "ysb_sync": (_I, [_P]),
    "ysb_drain": (_I, [_P, _I64, _I64, _I, C.POINTER(YsbCount), _U64, C.POINTER(_U64)]),
    "ysb_stats_get": (_I, [_P, C.POINTER(YsbStats)]),
    "ysb_flush_begin": (_I, [_P, _I64, _I64]),
    "ysb_flush_end": (_I, [_P, _I, C.POINTER(YsbCount), _U64, C.POINTER(_U64), C.POINTER(_I)]),
    "ysb_reset": (_I, [_P]),
    "ysb_ring_range": (_I, [_P, C.POINTER(_I64), C.POINTER(_U32)]),
    "ysb_ring_advance": (_I, [_P, _I64]),
    "ysb_kernel_time": (_I, [_P, C.POINTER(C.c_double), C.POINTER(_U64)]),
    "ysb_path_time": (_I, [_P, C.POINTER(C.c_double), C.POINTER(_U64), C.POINTER(_U64)]),
    "ysb_stream": (_P, [_P]),
    "ysb_launch_info": (_I, [_P, C.POINTER(YsbLaunchDesc)]),
    "ysb_record_info": (_I, [_P, C.POINTER(YsbRecordDesc), _PU32, _U64, _PU32, _U64]),
    "ysb_record_desc_size": (_U64, []),
    "ysb_layout_of_line": (_I, [C.c_char_p, _U64, _I, C.c_void_p, C.POINTER(_U32), C.POINTER(_U32)]),
    "ysb_device_alloc": (_I, [_P, _U64, C.POINTER(_P)]),
    "ysb_device_free": (_I, [_P, _P]),
    "ysb_memcpy_h2d": (_I, [_P, _P, _P, _U64]),
    "ysb_memcpy_d2h": (_I, [_P, _P, _P, _U64]),
    "ysb_group_unique_id": (_I, [C.c_char_p]),
    "ysb_group_init": (_I, [_P, _I, _I, C.c_char_p]),
    "ysb_group_reduce_scatter": (_I, [_P]),
    "ysb_group_exchange_pipelined": (_I, [_P]),
    "ysb_group_init_host": (_I, [_P, _I, _I, C.POINTER(YsbCollectives)]),
    "ysb_group_exchange_info": (_I, [_P, C.POINTER(YsbExchangeInfo), _I]),
    "ysb_exchange_info_size": (_U64, []),
    "ysb_exchange_plan": (_I, [C.c_void_p, _U32, _U32, C.c_void_p, C.POINTER(_U32), C.POINTER(_U32)]),
    "ysb_group_checksum": (_I, [_P, _I, _U32, C.c_void_p]),
    "ysb_group_owned": (_I, [_P, C.POINTER(_U32), C.POINTER(_U32)]),
    "ysb_group_info": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "ysb_ad_shard": (_U32, [C.c_char_p, _U32, _U32]),
    "ysb_group_block": (_I, [_U32, _I, _I, C.POINTER(_U32), C.POINTER(_U32)]),
    "ysb_route_lines": (_I, [_PU8, _U64, _PU32, _U64, _U32, _PU32, C.c_void_p]),
    "ysb_gen_default": (None, [C.POINTER(YsbGenParams)]),
    "ysb_gen_ids": (_I, [C.POINTER(YsbGenParams), _P, _P]),
    "ysb_gen_events_host": (_I, [C.POINTER(YsbGenParams), _U64, _U64, _PU8, _U64, _PU32, C.POINTER(_U64)]),
    "ysb_gen_events_host_mt": (_I, [C.POINTER(YsbGenParams), _U64, _U64, _PU8, _U64, _PU32, C.POINTER(_U64), _U32]),
    "ysb_gen_events_device": (_I, [_P, C.POINTER(YsbGenParams), _U64, _U64, _PU8, _U64, _PU32, C.POINTER(_U64)]),
    "ysb_gen_max_line_bytes": (_U64, [C.POINTER(YsbGenParams)]),
    "ysb_truth_accumulate": (_I, [_P, C.POINTER(YsbGenParams), _U64, _U64]),
    "ysb_truth_compare": (_I, [_P, C.POINTER(_U64), C.POINTER(_U64), C.POINTER(_U64)]),
    "ysb_truth_read": (_I, [_P, C.c_void_p, _U64, C.POINTER(_I64)]),
    "ysb_gen_dump": (_I, [C.POINTER(YsbGenParams), _U64, C.c_char_p]),
    "ysb_json_to_tbl": (_I, [_PU8, _U64, _PU32, _U64, _PU8, _U64, _PU32, C.POINTER(_U64)]),
    "ysb_gen_dump_shards": (_I, [C.POINTER(YsbGenParams), _U64, C.c_char_p, _U32]),
}



class ArrowSchema(C.Structure):
    """struct ArrowSchema of the Arrow C data interface."""


ArrowSchema._fields_ = [("format", C.c_char_p), ("name", C.c_char_p), ("metadata", C.c_char_p), ("flags", C.c_int64),
                        ("n_children", C.c_int64), ("children", C.POINTER(C.POINTER(ArrowSchema))),
                        ("dictionary", C.POINTER(ArrowSchema)), ("release", C.c_void_p), ("private_data", C.c_void_p)]


class ArrowArray(C.Structure):
    """struct ArrowArray of the Arrow C data interface."""


ArrowArray._fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
                       ("n_children", C.c_int64), ("buffers", C.POINTER(C.c_void_p)),
                       ("children", C.POINTER(C.POINTER(ArrowArray))), ("dictionary", C.POINTER(ArrowArray)),
                       ("release", C.c_void_p), ("private_data", C.c_void_p)]


class YsbArrowBinding(C.Structure):
    _fields_ = [("n_children", C.c_int64), ("child", C.c_int64 * 3), ("kind", C.c_uint32 * 3), ("reserved", C.c_uint32)]


class YsbArrowCol(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("data_first", C.c_uint32), ("validity", C.c_void_p), ("offsets", C.c_void_p),
                ("data", C.c_void_p), ("data_bytes", C.c_uint64), ("offset", C.c_uint64), ("validity_offset", C.c_uint64)]


class YsbArrowCols(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("validity", C.c_void_p), ("offset", C.c_uint64), ("col", YsbArrowCol * 3),
                ("dict", YsbArrowCol), ("dict_len", C.c_uint64)]


class YsbArrowRange(C.Structure):
    _fields_ = [("src", C.c_void_p), ("bytes", C.c_uint64), ("dst", C.c_uint64), ("col", C.c_uint32), ("what", C.c_uint32)]


class YsbArrowDesc(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("tiles", C.c_uint64), ("grid", C.c_uint32), ("resident_grid", C.c_uint32),
                ("per_lane_tiles", C.c_uint64), ("invalid_null", C.c_uint64), ("invalid_offsets", C.c_uint64),
                ("invalid_dict", C.c_uint64), ("kind", C.c_uint32 * 3), ("lds_counters", C.c_uint32),
                ("hbm_table", C.c_uint32), ("reserved", C.c_uint32)]


SIGNATURES.update({
    "ysb_arrow_bind": (_I, [C.POINTER(ArrowSchema), C.POINTER(YsbArrowBinding)]),
    "ysb_arrow_binding_size": (_U64, []),
    "ysb_arrow_cols_size": (_U64, []),
    "ysb_arrow_desc_size": (_U64, []),
    "ysb_arrow_plan": (_I, [C.POINTER(YsbArrowBinding), C.POINTER(ArrowArray), C.POINTER(YsbArrowRange), _U64,
                            C.POINTER(_U64), C.POINTER(_U64)]),
    "ysb_arrow_pack": (_I, [C.POINTER(YsbArrowBinding), C.POINTER(ArrowArray), C.c_void_p, _U64, C.POINTER(YsbArrowCols)]),
    "ysb_arrow_view": (_I, [C.POINTER(YsbArrowBinding), C.POINTER(ArrowArray), C.POINTER(YsbArrowCols)]),
    "ysb_arrow_count_host": (_I, [C.POINTER(YsbArrowCols), C.c_void_p, C.c_void_p, C.c_void_p, _U64, _I64, _U32, _U32,
                                  C.POINTER(_U64), C.POINTER(_U64), C.c_void_p, _U64, C.POINTER(_U64)]),
    "ysb_submit_arrow": (_I, [_P, _I, C.POINTER(YsbArrowBinding), C.POINTER(ArrowArray)]),
    "ysb_submit_arrow_device": (_I, [_P, C.POINTER(YsbArrowCols)]),
    "ysb_arrow_launch_info": (_I, [_P, C.POINTER(YsbArrowDesc)]),
})

ABI_VERSION = 6   # include/ysb_hip.h YSB_ABI_VERSION this binding is written against

_lib = None


class YsbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "?"), code, msg))
        self.code = code


def lib():
    """The loaded library.  Raises if the in-tree build is missing (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libysb_hip.so not built at %s: run `make -C streaming-benchmarks_amd` "
                              "(or __graft_entry__.build())" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        # the structs this binding lays out must be the library's (ysb_exchange_info grew in
        # ABI 4: an older caller's struct would be written past its end)
        if L.ysb_abi_version() != ABI_VERSION:
            raise ImportError("%s has ABI %d, this binding is written for ABI %d: rebuild the library"
                              % (LIB_PATH, L.ysb_abi_version(), ABI_VERSION))
        if L.ysb_exchange_info_size() != C.sizeof(YsbExchangeInfo):
            raise ImportError("ysb_exchange_info is %d bytes in the library, %d in this binding"
                              % (L.ysb_exchange_info_size(), C.sizeof(YsbExchangeInfo)))
        if L.ysb_record_desc_size() != C.sizeof(YsbRecordDesc):
            raise ImportError("ysb_record_desc is %d bytes in the library, %d in this binding"
                              % (L.ysb_record_desc_size(), C.sizeof(YsbRecordDesc)))
        if L.ysb_colcount_desc_size() != C.sizeof(YsbColcountDesc):
            raise ImportError("ysb_colcount_desc is %d bytes in the library, %d in this binding"
                              % (L.ysb_colcount_desc_size(), C.sizeof(YsbColcountDesc)))
        for fn, st in ((L.ysb_upsert_info_size, YsbUpsertInfo), (L.ysb_admap_desc_size, YsbAdmapDesc),
                       (L.ysb_parked_info_size, YsbParkedDesc), (L.ysb_lz4_desc_size, YsbLz4Desc),
                       (L.ysb_lz4_frame_desc_size, YsbLz4FrameDesc), (L.ysb_arrow_binding_size, YsbArrowBinding),
                       (L.ysb_arrow_cols_size, YsbArrowCols), (L.ysb_arrow_desc_size, YsbArrowDesc),
                       (L.ysb_join_info_size, YsbJoinInfo), (L.ysb_kafka_batch_size, YsbKafkaBatch),
                       (L.ysb_kafka_summary_size, YsbKafkaSummary), (L.ysb_kafka_verdict_size, YsbKafkaVerdict),
                       (L.ysb_kafka_counters_size, YsbKafkaCounters), (L.ysb_kafka_pack_opts_size, YsbKafkaPackOpts),
                       (L.ysb_kafka_desc_size, YsbKafkaDesc), (L.ysb_kafka_frame_size, YsbKafkaFrame),
                       (L.ysb_kafka_crc_desc_size, YsbKafkaCrcDesc),
                       (L.ysb_kafka_lz4_summary_size, YsbKafkaLz4Summary), (L.ysb_kafka_lz4_desc_size, YsbKafkaLz4Desc)):
            if fn() != C.sizeof(st):
                raise ImportError("%s is %d bytes in the library, %d in this binding"
                                  % (st.__name__, fn(), C.sizeof(st)))
        _lib = L
    return _lib


def check(rc, ctx=None):
    if rc != YSB_OK:
        msg = lib().ysb_last_error(ctx)
        raise YsbError(rc, msg.decode() if msg else "")
    return rc
