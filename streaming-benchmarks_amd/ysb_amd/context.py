"""YsbContext: one device context of the GPU advertising operator.

Mirrors the lifecycle of the reference operators it replaces
(flink-benchmarks/.../AdvertisingTopologyNative.java:438-533):
  RedisJoinBolt(Map) / open()         -> YsbContext(...) + load_ad_map(...)
  flatMap(...) per record             -> submit(...) / submit_device(...) per batch
  CampaignProcessorCommon.flushWindows -> drain(...)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import INT64_MIN, YsbConfig, YsbCount, YsbExchangeInfo, YsbLaunchDesc, YsbSegment, YsbStats, check, lib


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def device_count():
    """The HIP devices this process sees (ysb_device_count: hipGetDeviceCount, no framework's
    device query -- a torch build that cannot see the GPU does not change it)."""
    return int(lib().ysb_device_count())


def device_sync(device):
    """hipDeviceSynchronize on `device` through the library's own HIP runtime (ysb_device_sync):
    the bench's device-wide wait without initialising a framework's HIP runtime, which may be
    another one than the library's (ABI 5)."""
    check(lib().ysb_device_sync(int(device)), None)


def columns_layout(rows):
    """ysb_columns_layout_of: the fork's seven-column layout (WindowedArrowFormatBolter,
    AdvertisingTopologyNative.java:278-356) for a batch of `rows` rows, as a dict: rows,
    start (9 byte offsets: the columns, [7] the validity bitmap, [8] the total), width (7),
    image_bytes (the reference's file image = start[7])."""
    lay = _lib.YsbColumnsLayout()
    check(lib().ysb_columns_layout_of(int(rows), C.byref(lay)), None)
    return {"rows": lay.rows, "start": [int(v) for v in lay.start], "width": [int(v) for v in lay.width],
            "image_bytes": lay.image_bytes}


def columns_read_ranges(rows, n_rows, flags=0):
    """ysb_columns_read_ranges: the [(offset, bytes), ...] a columnar count of rows [0, n_rows)
    of a batch of `rows` rows reads -- columns 2 (ad_id), 4 (event_type) and 5 (event_time),
    then with YSB_COL_VALIDITY the bitmap words: what a caller must make visible to the device
    and what submit_columns copies."""
    off, nb, n = (C.c_uint64 * 4)(), (C.c_uint64 * 4)(), C.c_uint32()
    check(lib().ysb_columns_read_ranges(int(rows), int(n_rows), int(flags), off, nb, C.byref(n)), None)
    return [(int(off[i]), int(nb[i])) for i in range(n.value)]


def joined_layout(cap_rows, flags=0):
    """ysb_joined_layout_of: the columns ysb_join_device writes for cap_rows rows, as a dict:
    cap_rows, start (7 byte offsets: campaign, row, event_time, time_ok, key, key_len, [6] the
    total), width (6; 0 for a column the flags leave out), flags, n_cols."""
    lay = _lib.YsbJoinedLayout()
    check(lib().ysb_joined_layout_of(int(cap_rows), int(flags), C.byref(lay)), None)
    return {"cap_rows": lay.cap_rows, "start": [int(v) for v in lay.start], "width": [int(v) for v in lay.width],
            "flags": lay.flags, "n_cols": lay.n_cols}


def joined_columns(image, lay, rows):
    """Rows [0, rows) of the columns of a joined_layout buffer copied to host memory (a uint8
    array), as a dict of numpy arrays."""
    st = lay["start"]
    out = {"campaign": image[st[0]:st[0] + 4 * rows].view("<u4").copy(),
           "row": image[st[1]:st[1] + 4 * rows].view("<u4").copy(),
           "event_time": image[st[2]:st[2] + 8 * rows].view("<i8").copy(),
           "time_ok": image[st[3]:st[3] + rows].copy()}
    if lay["flags"] & _lib.YSB_JOIN_KEYS:
        out["key"] = image[st[4]:st[4] + 56 * rows].reshape(rows, 56).copy()
        out["key_len"] = image[st[5]:st[5] + rows].copy()
    return out


def rank_device(local_rank, n_visible):
    """The device a rank uses (one context per GPU): its LOCAL_RANK, unless the launcher left
    each process fewer visible devices (e.g. one per rank through HIP_VISIBLE_DEVICES): then
    the (LOCAL_RANK mod n_visible)-th.  With none visible the local rank is kept, so the
    context's open fails loudly instead of silently sharing device 0."""
    if n_visible <= 0:
        return local_rank
    return local_rank if local_rank < n_visible else local_rank % n_visible


class YsbContext:
    def __init__(self, device=0, n_campaigns=100, time_divisor_ms=10000, window_ring=1024,
                 max_batch_events=1 << 20, max_batch_bytes=256 << 20, ring_base_bucket=None,
                 overflow_capacity=1 << 20, timing=False, require_ip=False, lds_count=True,
                 sparse_fast_join=False, input_format="json", record_count=None, compact_first=False,
                 flat_first=False, layout_auto=True, strict=False, h2d_sdma=False):
        L = lib()
        cfg = YsbConfig()
        L.ysb_config_default(C.byref(cfg))
        cfg.time_divisor_ms = time_divisor_ms
        cfg.n_campaigns = n_campaigns
        cfg.window_ring = window_ring
        cfg.max_batch_events = max_batch_events
        cfg.max_batch_bytes = max_batch_bytes
        cfg.ring_base_bucket = INT64_MIN if ring_base_bucket is None else ring_base_bucket
        cfg.overflow_capacity = overflow_capacity
        cfg.flags = ((_lib.YSB_F_TIMING if timing else 0) | (_lib.YSB_F_REQUIRE_IP if require_ip else 0)
                     | (0 if lds_count else _lib.YSB_F_NO_LDS_COUNT)
                     | (_lib.YSB_F_SPARSE_FAST_JOIN if sparse_fast_join else 0)
                 | (_lib.YSB_F_FORMAT_TBL if input_format == "tbl" else 0)
                 | (_lib.YSB_F_COMPACT_FIRST if compact_first else 0)
                 | (_lib.YSB_F_FLAT_FIRST if flat_first else 0)
                 | (0 if layout_auto else _lib.YSB_F_LAYOUT_FIXED)
                 | (_lib.YSB_F_STRICT if strict else 0)
                 | (_lib.YSB_F_H2D_SDMA if h2d_sdma else 0)
                 | (0 if record_count is None else
                    _lib.YSB_F_RECORD_COUNT if record_count else _lib.YSB_F_NO_RECORD_COUNT))
        if input_format not in ("json", "tbl"):
            raise ValueError("input_format must be 'json' or 'tbl'")
        h = C.c_void_p()
        check(L.ysb_open(C.byref(h), device, C.byref(cfg)), None)
        self._h = h
        self.cfg = cfg
        self.device = device

    # -- lifecycle ---------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib().ysb_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc):
        return check(rc, self._h)

    # -- join table --------------------------------------------------------------------
    def load_ad_map(self, ad_ids, campaign_idx, shard=None):
        """ad_ids: sequence of str/bytes; campaign_idx: matching campaign indices.

        shard = (rank, nranks): load only the ads of this rank's ad_id-hash shard
        (ysb_load_ad_map_shard) -- the join table sharded 1/N per GPU
        for input that is pre-sharded by the same hash (bench.py's ranks,
        ysb_gen_dump_shards).  The library keeps the shard: a view of another shard's ad
        counts as stats()["foreign_shard"] (an error with strict=True), not as a join miss."""
        keys = [a.encode() if isinstance(a, str) else bytes(a) for a in ad_ids]
        rank, nranks = shard if shard is not None else (0, 1)
        if not 0 <= rank < nranks:
            raise ValueError("shard rank out of range")
        n = len(keys)
        arr = (C.c_char_p * max(n, 1))(*keys)
        lens = (C.c_uint32 * max(n, 1))(*[len(k) for k in keys])
        camp = (C.c_uint32 * max(n, 1))(*[int(c) for c in campaign_idx])
        self._c(lib().ysb_load_ad_map_shard(self._h, arr, lens, camp, n, rank, nranks))

    def load_ad_map_packed(self, keys, campaign_idx, key_len=36, shard=None):
        """keys: uint8 array of n * key_len bytes; campaign_idx: n uint32; shard as load_ad_map."""
        k = np.ascontiguousarray(keys, dtype=np.uint8)
        cidx = np.ascontiguousarray(campaign_idx, dtype=np.uint32)
        if k.size != cidx.size * key_len:
            raise ValueError("keys must hold n * key_len bytes")
        rank, nranks = shard if shard is not None else (0, 1)
        self._c(lib().ysb_load_ad_map_packed_shard(self._h, _ptr(k), key_len, _ptr(cidx), cidx.size, rank, nranks))

    # -- the live map ------------------------------------------------------------------
    @staticmethod
    def _id_arrays(ad_ids):
        keys = [a.encode() if isinstance(a, str) else bytes(a) for a in ad_ids]
        n = len(keys)
        return n, (C.c_char_p * max(n, 1))(*keys), (C.c_uint32 * max(n, 1))(*[len(k) for k in keys])

    @staticmethod
    def _upsert_info(info):
        return {n: getattr(info, n) for n, _ in _lib.YsbUpsertInfo._fields_}

    def upsert_ad_map(self, ad_ids, campaign_idx):
        """HashMap.put of each (ad id, campaign index) in order on the live device tables
        (ysb_ad_map_upsert): new ads are added, known ones re-pointed, in stream order between
        the batches submitted before and after.  Returns ysb_upsert_info as a dict (entries,
        foreign, duplicates, updated, inserted, cuckoo_first / _second / _moved / _left_out,
        rebuilt, partial, device_ms)."""
        n, arr, lens = self._id_arrays(ad_ids)
        camp = (C.c_uint32 * max(n, 1))(*[int(c) for c in campaign_idx])
        info = _lib.YsbUpsertInfo()
        self._c(lib().ysb_ad_map_upsert(self._h, arr, lens, camp, n, C.byref(info)))
        return self._upsert_info(info)

    def upsert_ad_map_packed(self, keys, campaign_idx, key_len=36):
        """upsert_ad_map for a uint8 array of n * key_len key bytes and n uint32 campaign indices."""
        k = np.ascontiguousarray(keys, dtype=np.uint8)
        cidx = np.ascontiguousarray(campaign_idx, dtype=np.uint32)
        if k.size != cidx.size * key_len:
            raise ValueError("keys must hold n * key_len bytes")
        info = _lib.YsbUpsertInfo()
        self._c(lib().ysb_ad_map_upsert_packed(self._h, _ptr(k), key_len, _ptr(cidx), cidx.size, C.byref(info)))
        return self._upsert_info(info)

    def lookup_ads(self, ad_ids):
        """(campaign, where) uint32 arrays of the ids in the live tables (ysb_ad_map_lookup):
        campaign 0xFFFFFFFF for an absent id; where 0 absent, 1 / 2 the cuckoo table's first /
        second slot or bucket, 3 the general table only."""
        n, arr, lens = self._id_arrays(ad_ids)
        camp, where = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        self._c(lib().ysb_ad_map_lookup(self._h, arr, lens, n, _ptr(camp), _ptr(where)))
        return camp, where

    def ad_map_info(self):
        """ysb_ad_map_info as a dict: keys, keys36, table_slots, ctable_slots, buckets, partial,
        shard_rank, shard_n."""
        d = _lib.YsbAdmapDesc()
        self._c(lib().ysb_ad_map_info(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in _lib.YsbAdmapDesc._fields_}

    # -- parked views ------------------------------------------------------------------
    @staticmethod
    def _parked_desc(d):
        return {n: getattr(d, n) for n, _ in _lib.YsbParkedDesc._fields_}

    def park_misses(self, capacity):
        """ysb_parked_enable: from now on a view whose ad is in no device table is parked (up to
        `capacity` records) instead of being counted as a join miss, until resolve_parked; 0
        turns parking off.  RedisAdCampaignCache's jedis.get half: see resolve_parked_with."""
        self._c(lib().ysb_parked_enable(self._h, int(capacity)))

    def parked_keys(self):
        """ysb_parked_keys: the distinct ad ids of the parked views, a list of bytes in no
        particular order."""
        n = C.c_uint64()
        self._c(lib().ysb_parked_keys(self._h, None, None, 0, C.byref(n)))
        if not n.value:
            return []
        keys = np.zeros(n.value * 56, dtype=np.uint8)
        lens = np.zeros(n.value, dtype=np.uint32)
        self._c(lib().ysb_parked_keys(self._h, _ptr(keys), _ptr(lens), n.value, C.byref(n)))
        return [keys[56 * i:56 * i + int(lens[i])].tobytes() for i in range(n.value)]

    def resolve_parked(self):
        """ysb_parked_resolve: every parked view against the join tables as they are now --
        counted as the scan would have counted it if its ad is there, a join miss if not.
        Returns ysb_parked_desc as a dict (capacity, parked, parked_total, dropped,
        resolved_joined / _missed / _time_errors, distinct_keys, distinct_ms, resolve_ms)."""
        d = _lib.YsbParkedDesc()
        self._c(lib().ysb_parked_resolve(self._h, C.byref(d)))
        return self._parked_desc(d)

    def parked_info(self):
        """ysb_parked_info as a dict (the fields of resolve_parked)."""
        d = _lib.YsbParkedDesc()
        self._c(lib().ysb_parked_info(self._h, C.byref(d)))
        return self._parked_desc(d)

    def resolve_parked_with(self, lookup):
        """The whole miss loop of RedisAdCampaignCache.execute for what is parked now:
        lookup(list of ad id bytes) returns, per key, a campaign index or None (the ad is
        unknown there too); the ads found are upserted and the log is resolved.  Returns
        resolve_parked's dict."""
        keys = self.parked_keys()
        if keys:
            found = [(k, c) for k, c in zip(keys, lookup(keys)) if c is not None]
            if found:
                self.upsert_ad_map([k for k, _ in found], [c for _, c in found])
        return self.resolve_parked()

    # -- batches -----------------------------------------------------------------------
    def slot_buffers(self, slot):
        b, o = C.c_void_p(), C.c_void_p()
        self._c(lib().ysb_slot_buffers(self._h, slot, C.byref(b), C.byref(o)))
        return b.value, o.value

    def submit(self, data, offsets, slot=0):
        """Host batch (bytes / uint8 array + uint32 line offsets), double-buffered slot."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        self._c(lib().ysb_submit(self._h, slot, _ptr(buf), buf.size, _ptr(off), off.size))

    def wait(self, slot):
        self._c(lib().ysb_wait(self._h, slot))

    def slot_capacity(self):
        """(max_bytes, max_events) of each pinned slot (ysb_slot_capacity)."""
        b, e = C.c_uint64(), C.c_uint64()
        self._c(lib().ysb_slot_capacity(self._h, C.byref(b), C.byref(e)))
        return b.value, e.value

    def submit_raw(self, data, slot=0):
        """Raw batch (ysb_submit_raw): whole lines as bytes, the line starts found on the GPU
        (readLine's terminators); the scan launches at the next call on the context."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        self._c(lib().ysb_submit_raw(self._h, slot, _ptr(buf), buf.size))

    def host_register(self, arr, nbytes=None):
        """ysb_host_register: pins and maps a host numpy array for zero-copy raw batches (the
        array must stay alive and unmoved until host_unregister or close).  nbytes: the length
        to register from arr's start when it is not arr.nbytes (a file mapping's whole pages)."""
        self._c(lib().ysb_host_register(self._h, C.c_void_p(arr.ctypes.data),
                                        arr.nbytes if nbytes is None else int(nbytes)))

    def host_unregister(self, arr):
        self._c(lib().ysb_host_unregister(self._h, C.c_void_p(arr.ctypes.data)))

    def rebase_table(self, time_at, lead_base):
        """ysb_rebase_table: per line (time digits' offset) | (bucket index << 16), uint32."""
        t = np.ascontiguousarray(time_at, dtype=np.uint32)
        self._c(lib().ysb_rebase_table(self._h, _ptr(t), t.size, int(lead_base)))

    def submit_raw_mapped(self, arr, offset, nbytes, slot=0, rebase=None):
        """ysb_submit_raw_mapped: the raw batch arr[offset:offset + nbytes] of a registered
        array, read in place by the device; rebase = (first_line, lead_shift) or None."""
        rb = _lib.YsbRebase(*rebase) if rebase is not None else None
        self._c(lib().ysb_submit_raw_mapped(self._h, slot, C.c_void_p(arr.ctypes.data + offset), nbytes,
                                            C.byref(rb) if rb is not None else None))

    def submit_mapped(self, arr, offset, nbytes, d_off, n, slot=0, rebase=None):
        """ysb_submit_mapped: arr[offset:offset + nbytes] of a registered array with its n line
        offsets already in device memory (d_off); rebase = (first_line, lead_shift) or None."""
        rb = _lib.YsbRebase(*rebase) if rebase is not None else None
        self._c(lib().ysb_submit_mapped(self._h, slot, C.c_void_p(arr.ctypes.data + offset), nbytes,
                                        C.c_void_p(d_off), n, C.byref(rb) if rb is not None else None))

    def split_lines_device(self, d_bytes, nbytes, d_off, cap):
        """ysb_split_lines_device: the line starts of a device batch into d_off; returns n."""
        n = C.c_uint64()
        self._c(lib().ysb_split_lines_device(self._h, C.c_void_p(d_bytes), nbytes, C.c_void_p(d_off), cap,
                                             C.byref(n)))
        return n.value

    def submit_raw_lz4(self, blocks, directory, slot=0):
        """ysb_submit_raw_lz4: a raw batch as LZ4 blocks (bytes / uint8 array) and their
        directory (ysb_amd.lz4.pack's: an (n, 2) uint32 array of comp_bytes | stored bit,
        raw_bytes); only the compressed bytes cross PCIe, the GPU decodes, splits and scans."""
        buf = np.frombuffer(blocks, dtype=np.uint8) if isinstance(blocks, (bytes, bytearray)) else np.ascontiguousarray(blocks, dtype=np.uint8)
        d = np.ascontiguousarray(directory, dtype=np.uint32).reshape(-1, 2)
        self._c(lib().ysb_submit_raw_lz4(self._h, slot, _ptr(buf), buf.size, _ptr(d), d.shape[0]))

    def submit_lz4_mapped(self, arr, offset, comp_bytes, directory, slot=0, d_off=None, n=0, rebase=None):
        """ysb_submit_lz4_mapped: the LZ4 blocks arr[offset:offset + comp_bytes] of a registered
        array, read in place by the device, with their directory (host memory, as
        submit_raw_lz4's).  d_off None: the GPU splits the decoded lines (n must be 0);
        otherwise d_off holds n line offsets into the decoded batch in device memory.
        rebase = (first_line, lead_shift) or None."""
        d = np.ascontiguousarray(directory, dtype=np.uint32).reshape(-1, 2)
        rb = _lib.YsbRebase(*rebase) if rebase is not None else None
        self._c(lib().ysb_submit_lz4_mapped(self._h, slot, C.c_void_p(arr.ctypes.data + offset), comp_bytes,
                                            _ptr(d), d.shape[0], C.c_void_p(d_off) if d_off else None, n,
                                            C.byref(rb) if rb is not None else None))

    def lz4_decode_device(self, d_comp, comp_bytes, directory, d_out, out_cap):
        """ysb_lz4_decode_device: the decode alone, device to device.  Returns (raw bytes, first
        bad block or None); a bad block does not raise here -- its output range is untouched."""
        d = np.ascontiguousarray(directory, dtype=np.uint32).reshape(-1, 2)
        raw, bad = C.c_uint64(), C.c_uint32()
        rc = lib().ysb_lz4_decode_device(self._h, C.c_void_p(d_comp), comp_bytes, _ptr(d), d.shape[0],
                                         C.c_void_p(d_out), out_cap, C.byref(raw), C.byref(bad))
        if rc != -5 or bad.value == 0xFFFFFFFF:   # (YSB_ERR_FORMAT with a bad block: the return value says it)
            self._c(rc)
        return raw.value, (None if bad.value == 0xFFFFFFFF else bad.value)

    def lz4_info(self):
        """ysb_lz4_info as a dict: the last compressed batch (batches, blocks, stored_blocks,
        comp_bytes, raw_bytes, bad_blocks, first_bad or None, decode_ms with timing=True)."""
        d = _lib.YsbLz4Desc()
        self._c(lib().ysb_lz4_info(self._h, C.byref(d)))
        out = {n: getattr(d, n) for n, _ in d._fields_}
        if out["first_bad"] == 0xFFFFFFFF:
            out["first_bad"] = None
        return out

    def submit_lz4_blocks(self, data, index, slot=0, more=False):
        """ysb_submit_lz4_blocks: a run of consecutive entries of a standard frame's index
        (ysb_amd.lz4.frame_index over `data`, bytes or a uint8 array) as one batch; the GPU
        measures, decodes, splits and scans.  more=True: the bytes behind the batch's last certain
        line terminator are carried in front of the next frame batch."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        idx = np.ascontiguousarray(index)
        self._c(lib().ysb_submit_lz4_blocks(self._h, slot, _ptr(buf), _ptr(idx), idx.size, 1 if more else 0))

    def submit_lz4_blocks_mapped(self, arr, index, slot=0, more=False):
        """ysb_submit_lz4_blocks_mapped: the same with the blocks read in place from a registered
        array (host_register); the index's offsets refer to arr."""
        idx = np.ascontiguousarray(index)
        self._c(lib().ysb_submit_lz4_blocks_mapped(self._h, slot, C.c_void_p(arr.ctypes.data), _ptr(idx), idx.size,
                                                   1 if more else 0))

    def lz4_set_decoder(self, decoder):
        """ysb_lz4_set_decoder: 0 by the batch's largest block, 1 always the one-wave kernel, 2
        always the several-wave kernel."""
        self._c(lib().ysb_lz4_set_decoder(self._h, decoder))

    def lz4_measure_device(self, d_base, index):
        """ysb_lz4_measure_device: the raw size of every block of a frame index (ysb_amd.lz4.
        frame_index's) whose offsets refer to the device buffer d_base.  Returns (raw sizes as a
        uint32 array with 0 for a bad block, first bad block or None); bad blocks do not raise."""
        idx = np.ascontiguousarray(index)
        raw, bad = np.zeros(max(idx.size, 1), dtype=np.uint32), C.c_uint32()
        rc = lib().ysb_lz4_measure_device(self._h, C.c_void_p(d_base), _ptr(idx), idx.size, _ptr(raw), C.byref(bad))
        if rc != -5 or bad.value == 0xFFFFFFFF:
            self._c(rc)
        return raw[:idx.size], (None if bad.value == 0xFFFFFFFF else bad.value)

    def lz4_decode_blocks_device(self, d_base, index, d_out, out_cap):
        """ysb_lz4_decode_blocks_device: measure + decode of a frame index's blocks, device to
        device.  Returns (raw bytes, first bad block or None); a bad block does not raise."""
        idx = np.ascontiguousarray(index)
        raw, bad = C.c_uint64(), C.c_uint32()
        rc = lib().ysb_lz4_decode_blocks_device(self._h, C.c_void_p(d_base), _ptr(idx), idx.size, C.c_void_p(d_out),
                                                out_cap, C.byref(raw), C.byref(bad))
        if rc != -5 or bad.value == 0xFFFFFFFF:
            self._c(rc)
        return raw.value, (None if bad.value == 0xFFFFFFFF else bad.value)

    def lz4_frame_info(self):
        """ysb_lz4_frame_info as a dict: the last measure / decode of frame blocks (blocks,
        stored_blocks, comp_bytes, raw_bytes, bad_blocks, first_bad or None, decoder, and with
        timing=True measure_ms and decode_ms)."""
        d = _lib.YsbLz4FrameDesc()
        self._c(lib().ysb_lz4_frame_info(self._h, C.byref(d)))
        out = {n: getattr(d, n) for n, _ in d._fields_}
        if out["first_bad"] == 0xFFFFFFFF:
            out["first_bad"] = None
        return out

    def submit_kafka(self, data, index, slot=0):
        """ysb_submit_kafka: whole Kafka record batches (bytes / a uint8 array) with their index
        (ysb_amd.kafka.index over `data`); the framed bytes cross PCIe, the GPU finds the values,
        gathers them and scans them.  A bad Kafka batch drops the slot batch (YSB_ERR_FORMAT at
        the call that would have launched it)."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        idx = np.ascontiguousarray(index)
        self._c(lib().ysb_submit_kafka(self._h, slot, _ptr(buf), buf.size, _ptr(idx), idx.size))

    def submit_kafka_mapped(self, arr, offset, nbytes, index, slot=0):
        """ysb_submit_kafka_mapped: arr[offset:offset + nbytes] of a registered array, read in
        place by the device; the index's offsets are relative to that range's start."""
        idx = np.ascontiguousarray(index)
        self._c(lib().ysb_submit_kafka_mapped(self._h, slot, C.c_void_p(arr.ctypes.data + offset), nbytes, _ptr(idx),
                                              idx.size))

    def kafka_unframe_device(self, d_bytes, nbytes, index, d_out, out_cap, d_line_off, off_cap):
        """ysb_kafka_unframe_device: the unframing alone, device to device.  Returns (records,
        value bytes); raises YsbError (YSB_ERR_FORMAT) for a bad batch -- kafka_info()["verdict"]
        then names it."""
        idx = np.ascontiguousarray(index)
        n, nb = C.c_uint64(), C.c_uint64()
        self._c(lib().ysb_kafka_unframe_device(self._h, C.c_void_p(d_bytes), nbytes, _ptr(idx), idx.size,
                                               C.c_void_p(d_out), out_cap, C.c_void_p(d_line_off), off_cap,
                                               C.byref(n), C.byref(nb)))
        return n.value, nb.value

    def submit_kafka_lz4(self, data, index, frames, blocks, slot=0):
        """ysb_submit_kafka_lz4: whole Kafka record batches, uncompressed or LZ4-compressed, with
        the three arrays of ysb_amd.kafka.index_lz4 over `data`; the wire bytes cross PCIe, the GPU
        inflates, unframes and scans them.  YSB_ERR_CAPACITY unless len(blocks) * 65536 fits
        max_batch_bytes."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        idx, fr, bl = np.ascontiguousarray(index), np.ascontiguousarray(frames), np.ascontiguousarray(blocks)
        self._c(lib().ysb_submit_kafka_lz4(self._h, slot, _ptr(buf), buf.size, _ptr(idx), _ptr(fr), idx.size, _ptr(bl),
                                           bl.size))

    def submit_kafka_lz4_mapped(self, arr, offset, nbytes, index, frames, blocks, slot=0):
        """ysb_submit_kafka_lz4_mapped: arr[offset:offset + nbytes] of a registered array, read in
        place by the device; the arrays' offsets are relative to that range's start."""
        idx, fr, bl = np.ascontiguousarray(index), np.ascontiguousarray(frames), np.ascontiguousarray(blocks)
        self._c(lib().ysb_submit_kafka_lz4_mapped(self._h, slot, C.c_void_p(arr.ctypes.data + offset), nbytes, _ptr(idx),
                                                  _ptr(fr), idx.size, _ptr(bl), bl.size))

    def kafka_unframe_lz4_device(self, d_bytes, nbytes, index, frames, blocks, d_out, out_cap, d_line_off, off_cap):
        """ysb_kafka_unframe_lz4_device: inflate and unframing alone, device to device.  Returns
        (records, value bytes); raises YsbError (YSB_ERR_FORMAT) for a bad batch --
        kafka_info()["verdict"] then names it (rule 8: a block, `record` its index)."""
        idx, fr, bl = np.ascontiguousarray(index), np.ascontiguousarray(frames), np.ascontiguousarray(blocks)
        n, nb = C.c_uint64(), C.c_uint64()
        self._c(lib().ysb_kafka_unframe_lz4_device(self._h, C.c_void_p(d_bytes), nbytes, _ptr(idx), _ptr(fr), idx.size,
                                                   _ptr(bl), bl.size, C.c_void_p(d_out), out_cap,
                                                   C.c_void_p(d_line_off), off_cap, C.byref(n), C.byref(nb)))
        return n.value, nb.value

    def kafka_set_crc(self, mode):
        """ysb_kafka_set_crc: 0 off (the default), 1 (ysb_amd.kafka.CRC_DEVICE) every indexed
        batch's CRC-32C verified on the GPU by the Kafka submits and unframe calls; a batch whose
        CRC differs is bad by rule 9.  Kept across reset()."""
        self._c(lib().ysb_kafka_set_crc(self._h, int(mode)))

    def kafka_set_codecs(self, codecs=("lz4",)):
        """ysb_kafka_set_codecs: which codecs the compressed Kafka entries take -- names
        ("lz4", "snappy"; none and lz4 are always in) or the mask itself.  Kept across reset."""
        from . import kafka
        if isinstance(codecs, int):
            mask = codecs
        else:
            if any(n not in kafka.CODECS for n in codecs):
                raise ValueError("codecs %r: of %s" % (codecs, sorted(kafka.CODECS)))
            mask = kafka.CODECS["none"] | kafka.CODECS["lz4"]
            for n in codecs:
                mask |= kafka.CODECS[n]
        self._c(lib().ysb_kafka_set_codecs(self._h, mask))

    def kafka_test_inflated_cap(self, nbytes):
        """ysb_kafka_test_inflated_cap (test support): a smaller limit in the plan kernel's test of a
        batch's inflated extent; 0 restores the buffer's size."""
        self._c(lib().ysb_kafka_test_inflated_cap(self._h, int(nbytes)))

    def kafka_crc_device(self, d_bytes, nbytes, index):
        """ysb_kafka_crc_device: the CRC kernel alone over the indexed batches of a device buffer.
        Returns (computed, stored) as uint32 arrays, one entry per batch."""
        idx = np.ascontiguousarray(index)
        got, want = np.zeros(max(idx.size, 1), dtype=np.uint32), np.zeros(max(idx.size, 1), dtype=np.uint32)
        self._c(lib().ysb_kafka_crc_device(self._h, C.c_void_p(d_bytes), nbytes, _ptr(idx), idx.size, _ptr(got), _ptr(want)))
        return got[:idx.size], want[:idx.size]

    def kafka_crc_info(self, check=True):
        """ysb_kafka_crc_info as a dict: the last call that verified CRCs on the device (calls,
        mode, batches, bytes, bad_batches, first_bad or None, stored, computed, grid_waves, and
        with timing=True crc_ms)."""
        d = _lib.YsbKafkaCrcDesc()
        rc = lib().ysb_kafka_crc_info(self._h, C.byref(d))
        if check:
            self._c(rc)
        out = {n: getattr(d, n) for n, _ in d._fields_}
        if out["first_bad"] == 0xFFFFFFFF:
            out["first_bad"] = None
        return out

    def kafka_lz4_info(self, check=True):
        """ysb_kafka_lz4_info as a dict: the inflate half of the last compressed Kafka call settled
        (calls, blocks, stored_blocks, compressed_batches, wire_bytes, inflated_bytes, bad_blocks,
        decoder, inflated_buffer_bytes -- 0 until a compressed call allocates one --, and with
        timing=True measure_ms, plan_ms, decode_ms)."""
        d = _lib.YsbKafkaLz4Desc()
        rc = lib().ysb_kafka_lz4_info(self._h, C.byref(d))
        if check:
            self._c(rc)
        return {n: getattr(d, n) for n, _ in d._fields_}

    def kafka_info(self, check=True):
        """ysb_kafka_info as a dict: the last Kafka call settled (calls, batches, records,
        null_values, keyed, headers, control_skipped, framed_bytes, value_bytes, window_bytes, the
        verdict as a dict with first_bad None for a good call, and with timing=True walk_ms,
        base_ms, gather_ms).  check=False: a sticky error of an earlier batch does not raise."""
        d = _lib.YsbKafkaDesc()
        rc = lib().ysb_kafka_info(self._h, C.byref(d))
        if check:
            self._c(rc)
        out = {n: getattr(d, n) for n, _ in d._fields_ if n != "verdict"}
        v = {n: getattr(d.verdict, n) for n, _ in d.verdict._fields_}
        if v["first_bad"] == 0xFFFFFFFF:
            v["first_bad"] = None
        out["verdict"] = v
        return out

    def copy_time(self):
        """(total ms, copies, bytes) of the slot H2D copies since the last call (timing=True)."""
        t, k, b = C.c_double(), C.c_uint64(), C.c_uint64()
        self._c(lib().ysb_copy_time(self._h, C.byref(t), C.byref(k), C.byref(b)))
        return t.value, k.value, b.value

    def submit_device(self, d_bytes, nbytes, d_off, n):
        self._c(lib().ysb_submit_device(self._h, C.c_void_p(d_bytes), nbytes, C.c_void_p(d_off), n))

    def submit_device_segments(self, segs):
        """Several device batches [(d_bytes, nbytes, d_off, n), ...] in one kernel launch."""
        arr = (YsbSegment * max(len(segs), 1))()
        for i, (d_b, nb, d_o, n) in enumerate(segs):
            arr[i] = YsbSegment(d_b, nb, d_o, n)
        self._c(lib().ysb_submit_device_segments(self._h, arr, len(segs)))

    def sync(self):
        self._c(lib().ysb_sync(self._h))

    # -- columnar decode ---------------------------------------------------------------
    def decode_columns_device(self, d_bytes, nbytes, d_off, n, d_out, batch_rows, stamp=10, flags=0):
        """ysb_decode_columns_device: lines [0, n) of a device batch into rows [0, n) of the
        seven columns and the validity bitmap of d_out (columns_layout(batch_rows)["start"][8]
        bytes of HBM).  Returns the info as a dict: rows, valid, fast_rows, kernel_ms."""
        info = _lib.YsbDecodeInfo()
        self._c(lib().ysb_decode_columns_device(self._h, C.c_void_p(d_bytes), nbytes, C.c_void_p(d_off), n,
                                                C.c_void_p(d_out), batch_rows, int(stamp), int(flags),
                                                C.byref(info)))
        return {k: getattr(info, k) for k, _ in _lib.YsbDecodeInfo._fields_}

    def decode_columns(self, data, offsets, batch_rows=None, **kw):
        """Host batch (bytes / uint8 array + uint32 line offsets) decoded on the device:
        allocates, copies, decodes and returns (image: uint8[start[8]], valid: bool[n], info).
        The image is zero wherever the decode writes nothing (padding, rows past n).
        batch_rows defaults to the number of lines; kw: stamp, flags."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        n = off.size
        rows = max(n, 1) if batch_rows is None else int(batch_rows)
        total = columns_layout(rows)["start"][8]
        image = np.zeros(total, dtype=np.uint8)
        d_b, d_o, d_out = self.device_alloc(buf.size), self.device_alloc(4 * n), self.device_alloc(total)
        try:
            if buf.size:
                self.h2d(d_b, buf)
            if n:
                self.h2d(d_o, off)
            self.h2d(d_out, image)
            info = self.decode_columns_device(d_b, buf.size, d_o, n, d_out, rows, **kw)
            self.d2h(image, d_out)
        finally:
            for p in (d_b, d_o, d_out):
                self.device_free(p)
        words = image[columns_layout(rows)["start"][7]:][:8 * ((n + 63) // 64)].view("<u8")
        valid = ((words[np.arange(n) // 64] >> (np.arange(n) % 64).astype(np.uint64)) & np.uint64(1)).astype(np.bool_)
        return image, valid, info

    # -- joined views ------------------------------------------------------------------
    def join_device(self, d_bytes, nbytes, d_off, n, d_out, cap_rows, flags=0):
        """ysb_join_device: the joined views of lines [0, n) of a device batch -- RedisJoinBolt's
        Tuple3 stream (AdvertisingTopologyNative.java:460-474) -- in source order as the columns
        of d_out (joined_layout(cap_rows, flags)["start"][6] bytes of HBM).  Returns the info as
        a dict: events, views, joined, join_misses, parse_errors, time_errors, foreign_shard,
        rows_written, fast_rows, tiles, grid, max_grid, join_ms, prefix_ms, pack_ms.  With more
        joined views than cap_rows the first cap_rows rows are written and the YsbError
        (YSB_ERR_CAPACITY) raised carries the complete dict as its `info`."""
        info = _lib.YsbJoinInfo()
        rc = lib().ysb_join_device(self._h, C.c_void_p(d_bytes), nbytes, C.c_void_p(d_off), n, C.c_void_p(d_out),
                                   int(cap_rows), int(flags), C.byref(info))
        out = {k: getattr(info, k) for k, _ in _lib.YsbJoinInfo._fields_}
        try:
            self._c(rc)
        except _lib.YsbError as e:
            if e.code == -4 and out["joined"] > int(cap_rows):
                e.info = out
            raise
        return out

    def join(self, data, offsets, keys=False, cap_rows=None):
        """Host batch (bytes / uint8 array + uint32 line offsets) joined on the device: allocates,
        copies, joins and returns (columns, info), columns a dict of numpy arrays of info["joined"]
        rows each: campaign uint32, row uint32, event_time int64, time_ok uint8 and, with keys,
        key uint8[rows, 56] and key_len uint8.  cap_rows defaults to the number of lines, which
        always suffices."""
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(offsets, dtype=np.uint32)
        n = off.size
        cap = n if cap_rows is None else int(cap_rows)
        flags = _lib.YSB_JOIN_KEYS if keys else 0
        lay = joined_layout(cap, flags)
        image = np.zeros(max(lay["start"][6], 16), dtype=np.uint8)
        d_b, d_o, d_out = self.device_alloc(max(buf.size, 16)), self.device_alloc(max(4 * n, 16)), self.device_alloc(image.size)
        try:
            if buf.size:
                self.h2d(d_b, buf)
            if n:
                self.h2d(d_o, off)
            self.h2d(d_out, image)
            info = self.join_device(d_b, buf.size, d_o, n, d_out, cap, flags)
            self.d2h(image, d_out)
        finally:
            for p in (d_b, d_o, d_out):
                self.device_free(p)
        return joined_columns(image, lay, info["rows_written"]), info

    # -- columnar count ----------------------------------------------------------------
    def submit_columns_device(self, d_cols, batch_rows, n_rows, flags=0):
        """ysb_submit_columns_device: rows [0, n_rows) of a device-resident column batch
        (columns_layout(batch_rows); with YSB_COL_VALIDITY up to start[8]) through filter, join
        and window count.  Asynchronous on the compute stream."""
        self._c(lib().ysb_submit_columns_device(self._h, C.c_void_p(d_cols), int(batch_rows), int(n_rows),
                                                int(flags)))

    def submit_columns(self, image, batch_rows, n_rows, slot=0, flags=0):
        """ysb_submit_columns: the host form.  image: a uint8 array (or bytes) holding the batch,
        or the address of the slot's own pinned buffer (slot_buffers(slot)[0]); only
        columns_read_ranges' bytes are copied.  wait(slot) before the slot is rewritten."""
        if isinstance(image, int):
            ptr = C.c_void_p(image)
        else:
            image = np.frombuffer(image, dtype=np.uint8) if isinstance(image, (bytes, bytearray)) else np.ascontiguousarray(image, dtype=np.uint8)
            ptr = _ptr(image)
        self._c(lib().ysb_submit_columns(self._h, slot, ptr, int(batch_rows), int(n_rows), int(flags)))

    def columns_launch_info(self):
        """The last columnar launch (ysb_columns_launch_info): rows, lds_counters, hbm_table,
        java_order, validity.  Raises YSB_ERR_STATE before the first one."""
        d = _lib.YsbColcountDesc()
        self._c(lib().ysb_columns_launch_info(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in _lib.YsbColcountDesc._fields_}

    # -- Arrow record batches ------------------------------------------------------------
    def submit_arrow(self, batch, slot=0, binding=None):
        """ysb_submit_arrow: the host form.  batch: an object with __arrow_c_array__ (the
        PyCapsule protocol), a pyarrow RecordBatch (_export_to_c), or ysb_amd.arrow.batch()'s
        output.  Only the rows' bytes are copied.  The batch is kept alive until wait(slot) or
        the slot's next submit_arrow; returns the binding (pass it back for the next batch of
        the same schema)."""
        from . import arrow
        ex = arrow.export(batch)
        if binding is None:
            binding = arrow.bind(ex.schema)
        self._c(lib().ysb_submit_arrow(self._h, slot, C.byref(binding), C.byref(ex.array)))
        if not hasattr(self, "_arrow_live"):
            self._arrow_live = {}
        self._arrow_live[slot] = ex
        return binding

    def submit_arrow_device(self, cols):
        """ysb_submit_arrow_device: a ysb_arrow_cols (ysb_amd.arrow.cols) of device pointers at any
        alignment.  Asynchronous on the compute stream."""
        self._c(lib().ysb_submit_arrow_device(self._h, C.byref(cols)))

    def arrow_launch_info(self):
        """The last Arrow launch (ysb_arrow_launch_info; waits for it): rows, tiles, grid,
        resident_grid, per_lane_tiles, invalid_null / _offsets / _dict, kind, lds_counters,
        hbm_table.  Raises YSB_ERR_STATE before the first one."""
        d = _lib.YsbArrowDesc()
        self._c(lib().ysb_arrow_launch_info(self._h, C.byref(d)))
        out = {n: getattr(d, n) for n, _ in _lib.YsbArrowDesc._fields_ if n != "reserved"}
        out["kind"] = tuple(d.kind)
        return out

    # -- results -----------------------------------------------------------------------
    def drain(self, bucket_lo=INT64_MIN, bucket_hi=(1 << 63) - 1, clear=False):
        """Returns {(campaign, window_ms): count} for buckets in [bucket_lo, bucket_hi)."""
        n = C.c_uint64()
        self._c(lib().ysb_drain(self._h, bucket_lo, bucket_hi, 0, None, 0, C.byref(n)))
        rows = (YsbCount * max(n.value, 1))()
        self._c(lib().ysb_drain(self._h, bucket_lo, bucket_hi, int(clear), rows, n.value, C.byref(n)))
        return {(rows[i].campaign, rows[i].window_ms): rows[i].count for i in range(n.value)}

    def flush_begin(self, bucket_lo=INT64_MIN, bucket_hi=(1 << 63) - 1):
        """ysb_flush_begin: the ring's deltas of [bucket_lo, bucket_hi) compacted behind every
        submitted batch, without waiting."""
        self._c(lib().ysb_flush_begin(self._h, bucket_lo, bucket_hi))

    def flush_end(self, wait=True):
        """The oldest begun flush as ({(campaign, window_ms): count}, more), or None while it is
        pending (wait=False)."""
        n, more = C.c_uint64(), C.c_int()
        rc = lib().ysb_flush_end(self._h, int(wait), None, 0, C.byref(n), C.byref(more))
        if rc == _lib.YSB_PENDING:
            return None
        self._c(rc)
        rows = (YsbCount * max(n.value, 1))()
        self._c(lib().ysb_flush_end(self._h, 1, rows, n.value, C.byref(n), C.byref(more)))
        return {(rows[i].campaign, rows[i].window_ms): rows[i].count for i in range(n.value)}, bool(more.value)

    def drain_buckets(self, **kw):
        """Same as drain() keyed by (campaign, bucket) instead of window_ms."""
        d = self.cfg.time_divisor_ms
        return {(c, w // d): v for (c, w), v in self.drain(**kw).items()}

    def stats(self):
        s = YsbStats()
        self._c(lib().ysb_stats_get(self._h, C.byref(s)))
        return {n: getattr(s, n) for n, _ in YsbStats._fields_}

    def reset(self):
        self._c(lib().ysb_reset(self._h))

    def ring_range(self):
        lo, w = C.c_int64(), C.c_uint32()
        self._c(lib().ysb_ring_range(self._h, C.byref(lo), C.byref(w)))
        return lo.value, w.value

    def ring_advance(self, new_lo):
        """Moves the ring to [new_lo, new_lo + W); leaving buckets go to the exact host list."""
        self._c(lib().ysb_ring_advance(self._h, int(new_lo)))

    def kernel_time(self):
        """(total ms, launches) of the scan kernel since the last call (needs timing=True)."""
        t, k = C.c_double(), C.c_uint64()
        self._c(lib().ysb_kernel_time(self._h, C.byref(t), C.byref(k)))
        return t.value, k.value

    def path_time(self):
        """(total ms, launches, record-mode launches so far): the whole device sequence of
        the launches the last kernel_time() call collected (scan + general path + record
        mode's partition and count kernels)."""
        t, k, r = C.c_double(), C.c_uint64(), C.c_uint64()
        self._c(lib().ysb_path_time(self._h, C.byref(t), C.byref(k), C.byref(r)))
        return t.value, k.value, r.value

    def launch_info(self):
        """The scan instantiation of the last launch: layout (0 generator, 1 compact, 2 flat,
        3 learned order, 4 per-tile dispatch), record_mode, hbm_table, tbl."""
        d = YsbLaunchDesc()
        self._c(lib().ysb_launch_info(self._h, C.byref(d)))
        return {n: getattr(d, n) for n, _ in YsbLaunchDesc._fields_}

    def record_info(self, arrays=True):
        """(descriptor, rec_n, runs) of the last record-mode launch (ysb_record_info): the plan
        as a dict (w_log2, blk_shift, n_blocks, sub_log2, bins, cap, grid, slices, area, part,
        delta_bound, dirty), rec_n uint32 [grid][bins] (records stored per sub-buffer) and runs
        uint32 [n_blocks][slices][2] ({offset, length} of each block's run per partition slice).
        A sync, not a fold.  arrays=False: the descriptor only, (dict, None, None).  Raises
        YSB_ERR_STATE before the first record-mode launch."""
        d = _lib.YsbRecordDesc()
        self._c(lib().ysb_record_info(self._h, C.byref(d), None, 0, None, 0))
        desc = {n: getattr(d, n) for n, _ in _lib.YsbRecordDesc._fields_ if n != "reserved"}
        if not arrays:
            return desc, None, None
        rec_n = np.zeros((d.grid, d.bins), dtype=np.uint32)
        runs = np.zeros((d.n_blocks, d.slices, 2), dtype=np.uint32)
        self._c(lib().ysb_record_info(self._h, C.byref(d), _ptr(rec_n), rec_n.size, _ptr(runs), runs.size))
        return desc, rec_n, runs

    def stream(self):
        s = lib().ysb_stream(self._h)
        if not s:   # a pending raw batch could not launch (sticky until reset)
            raise _lib.YsbError(-3, (lib().ysb_last_error(self._h) or b"").decode())
        return s

    # -- device memory -----------------------------------------------------------------
    def device_alloc(self, nbytes):
        p = C.c_void_p()
        self._c(lib().ysb_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def device_free(self, p):
        self._c(lib().ysb_device_free(self._h, C.c_void_p(p)))

    def h2d(self, d_dst, arr):
        arr = np.ascontiguousarray(arr)
        self._c(lib().ysb_memcpy_h2d(self._h, C.c_void_p(int(d_dst)), _ptr(arr), arr.nbytes))

    def d2h(self, arr, d_src):
        self._c(lib().ysb_memcpy_d2h(self._h, _ptr(arr), C.c_void_p(int(d_src)), arr.nbytes))
        return arr

    # -- multi-GPU ------------------------------------------------------------------------
    @staticmethod
    def group_unique_id() -> bytes:
        buf = C.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        check(lib().ysb_group_unique_id(buf), None)
        return buf.raw

    def group_init(self, rank, nranks, uid: bytes):
        self._c(lib().ysb_group_init(self._h, rank, nranks, C.create_string_buffer(uid, _lib.UNIQUE_ID_BYTES)))

    callback_error = None   # the last exception a group_init_host_fns callable raised

    def group_init_host_fns(self, rank, nranks, allreduce_max, reduce_scatter_sum):
        """ysb_group_init_host over two Python callables on numpy views of the library's host
        buffers (a transport of the caller's; a test that plays the other ranks itself):
          allreduce_max(buf: uint64[n])  -- elementwise max over the ranks, in place;
          reduce_scatter_sum(send, count, width) -> count cells -- send is the read-only uint8
            view of this rank's nranks * count cells of `width` bytes (every owner's block);
            the return value is this rank's block summed over the ranks, as unsigned cells.
        An exception in a callable never crosses the C frame: it is kept in
        self.callback_error and the library call fails (YSB_ERR_RCCL)."""
        cell = {1: np.uint8, 4: np.uint32, 8: np.uint64}

        def amax(_user, buf, n):
            try:
                allreduce_max(np.ctypeslib.as_array(buf, shape=(n,)))
                return 0
            except BaseException as e:   # noqa: BLE001 (a failing callback fails the call)
                self.callback_error = e
                return 1

        def rsum(_user, send, recv, count, width):
            try:
                nb = count * width
                s_ = np.frombuffer((C.c_char * (nb * nranks)).from_address(send), dtype=np.uint8)
                s_.flags.writeable = False
                out = np.ascontiguousarray(reduce_scatter_sum(s_, count, width), dtype=cell[width])
                if out.size != count:
                    raise ValueError("reduce_scatter_sum returned %d cells, not %d" % (out.size, count))
                C.memmove(recv, out.ctypes.data, nb)
                return 0
            except BaseException as e:   # noqa: BLE001
                self.callback_error = e
                return 1
        self.callback_error = None
        self._coll = _lib.YsbCollectives(_lib.ALLREDUCE_MAX_FN(amax), _lib.REDUCE_SCATTER_FN(rsum), None)
        self._c(lib().ysb_group_init_host(self._h, rank, nranks, C.byref(self._coll)))

    def group_init_host(self, rank, nranks, dist):
        """ysb_group_init_host over torch.distributed (e.g. gloo) as the transport: the
        library's exchange with the process group's collectives on host memory (N ranks on
        one GPU, where RCCL refuses two ranks per device)."""
        import torch

        def amax(a):
            t = torch.from_numpy((a ^ np.uint64(1 << 63)).view(np.int64).copy())
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            a[:] = t.numpy().view(np.uint64) ^ np.uint64(1 << 63)

        def rsum(send, count, width):
            # (torch has no unsigned 32 / 64-bit sums: two's complement adds the same bits)
            s_ = send.view({1: np.uint8, 4: np.int32, 8: np.int64}[width]).copy()
            out = torch.zeros(count, dtype={1: torch.uint8, 4: torch.int32, 8: torch.int64}[width])
            dist.reduce_scatter_tensor(out, torch.from_numpy(s_))
            return out.numpy().view({1: np.uint8, 4: np.uint32, 8: np.uint64}[width])
        self.group_init_host_fns(rank, nranks, amax, rsum)

    def group_reduce_scatter(self):
        """The complete exchange: every pending count reaches its owner."""
        self._c(lib().ysb_group_reduce_scatter(self._h))

    def group_exchange_pipelined(self):
        """The streaming exchange (ysb_group_exchange_pipelined): no host wait, packs with the
        previous call's plan; what it leaves pending travels with a later exchange."""
        self._c(lib().ysb_group_exchange_pipelined(self._h))

    def exchange_info(self, reset=False):
        """Exchange accounting (ysb_group_exchange_info): exchanges, bytes, ms, last_buckets,
        last_width, full_ring_bytes, critical_ms, rs_ms, exposed_ms."""
        x = YsbExchangeInfo()
        self._c(lib().ysb_group_exchange_info(self._h, C.byref(x), int(reset)))
        return {n: getattr(x, n) for n, _ in YsbExchangeInfo._fields_}

    def checksum(self, what, nranks=1):
        """Linear table checksums (ysb_group_checksum): what = 'truth' / 'pending' (one per
        owner block of nranks) or 'owned' (this rank's owned table)."""
        code = {"truth": _lib.YSB_SUM_TRUTH_BLOCKS, "pending": _lib.YSB_SUM_PENDING_BLOCKS,
                "owned": _lib.YSB_SUM_OWNED}[what]
        out = np.zeros(max(nranks, 1), dtype=np.uint64)
        self._c(lib().ysb_group_checksum(self._h, code, nranks, _ptr(out)))
        return [int(v) for v in (out[:1] if what == "owned" else out[:nranks])]

    def group_info(self):
        """(rank, nranks) as RCCL's communicator reports them (ncclCommUserRank / ncclCommCount)."""
        r, n = C.c_int(), C.c_int()
        self._c(lib().ysb_group_info(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def group_owned(self):
        lo, hi = C.c_uint32(), C.c_uint32()
        self._c(lib().ysb_group_owned(self._h, C.byref(lo), C.byref(hi)))
        return lo.value, hi.value

    # -- generator on this device ------------------------------------------------------------
    def gen_events_device(self, params, first, n, d_out, cap, d_off):
        nb = C.c_uint64()
        self._c(lib().ysb_gen_events_device(self._h, C.byref(params.c), first, n, C.c_void_p(d_out), cap,
                                            C.c_void_p(d_off), C.byref(nb)))
        return nb.value

    def truth_accumulate(self, params, first, n):
        self._c(lib().ysb_truth_accumulate(self._h, C.byref(params.c), first, n))

    def truth_read(self):
        """(truth table [n_campaigns][W] uint64, ring base bucket): the generator truth."""
        out = np.zeros((self.cfg.n_campaigns, self.cfg.window_ring), dtype=np.uint64)
        lo = C.c_int64()
        self._c(lib().ysb_truth_read(self._h, _ptr(out), out.size, C.byref(lo)))
        return out, lo.value

    def truth_compare(self):
        m, t, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._c(lib().ysb_truth_compare(self._h, C.byref(m), C.byref(t), C.byref(r)))
        return m.value, t.value, r.value
