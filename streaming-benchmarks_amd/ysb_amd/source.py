"""The events file as the reference's source reads it, handed to the GPU in place.

FileBasedDataSource mirrors `FileBasedDataSource.run` (flink-benchmarks/.../
AdvertisingTopologyNative.java:144-165: a BufferedReader over the events file, one record
per readLine) and the native runner's in-place mode (host/ysb_topology.cpp
`FileBasedDataSource::nextMapped`): the file is mapped read-only, the mapping registered with
the context once (ysb_host_register), and each batch -- the whole lines that fit in the
slot, cut where readLine cuts ("\\n", "\\r\\n", a lone "\\r") -- is submitted where it lies
(ysb_submit_raw_mapped: the copy kernel reads it over PCIe at any byte alignment and the GPU
splits its lines).  No byte of the file passes through a host copy.
"""
import mmap
import os

import numpy as np

PAGE = mmap.PAGESIZE


def complete_end(buf, start: int, have: int, at_eof: bool) -> int:
    """The end (relative to start) of the complete lines among buf[start:start + have]: up to
    the last terminator, everything at end of file; a '\\r' that ends the window may still be
    followed by '\\n', so it waits (FileBasedDataSource::completeEnd)."""
    if at_eof:
        return have
    q = have
    while q > 0:
        c = buf[start + q - 1]
        if c == 0x0A or (c == 0x0D and q < have):
            return q
        q -= 1
    raise ValueError("a line is longer than the batch buffer")


class FileBasedDataSource:
    """The events file, mapped read-only: `ranges(cap)` yields (offset, nbytes) of whole-line
    batches, back to back; `run(ctx, cap)` registers the mapping and submits every batch in
    place on alternating slots."""

    def __init__(self, path: str):
        self.path = path
        self.size = os.path.getsize(path)
        self._mm = None
        self.data = np.zeros(0, dtype=np.uint8)
        if self.size:
            with open(path, "rb") as f:
                self._mm = mmap.mmap(f.fileno(), 0, flags=mmap.MAP_SHARED, prot=mmap.PROT_READ)
            self.data = np.frombuffer(self._mm, dtype=np.uint8)
        self.bytes_read = 0
        self.batches = 0

    @property
    def mapping_bytes(self) -> int:
        """The registrable length: the mapping's whole pages (the copy reads whole 16-byte
        vectors, so the last batch may read past the file's end inside its last page)."""
        return (self.size + PAGE - 1) // PAGE * PAGE

    def ranges(self, cap: int):
        if cap <= 0:
            raise ValueError("cap must be positive")
        pos = 0
        while pos < self.size:
            have = min(cap, self.size - pos)
            end = complete_end(self.data, pos, have, pos + have >= self.size)
            yield pos, end
            pos += end

    def run(self, ctx, cap: int, rebase=None):
        """Every batch of the file through ctx (a YsbContext), in place; returns the bytes
        submitted.  At most two batches in flight (ysb_wait on the slot about to be reused)."""
        if not self.size:
            return 0
        ctx.host_register(self.data, self.mapping_bytes)
        try:
            slot = 0
            for off, nb in self.ranges(cap):
                ctx.submit_raw_mapped(self.data, off, nb, slot=slot)
                slot ^= 1
                ctx.wait(slot)
                self.bytes_read += nb
                self.batches += 1
            ctx.sync()
        finally:
            ctx.host_unregister(self.data)
        return self.bytes_read

    def close(self):
        self.data = np.zeros(0, dtype=np.uint8)
        if self._mm is not None:
            try:
                self._mm.close()
            except BufferError:   # a caller still holds a view of the mapping: it stays until freed
                pass
            self._mm = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class Lz4FileDataSource:
    """A compressed replay file -- the library's container (ysb_gen --lz4, ysb_amd.lz4.write_file:
    header, directory, blocks) or a standard LZ4 frame (lz4 -B4 -BI, ysb_gen --lz4-frame), told
    apart by magic --, mapped read-only: `runs(cap)` yields (offset into the mapping, compressed bytes,
    first block, blocks) of runs of whole blocks whose compressed and decoded sizes both fit
    cap; `run(ctx, cap)` registers the mapping and submits every run where it lies
    (ysb_submit_lz4_mapped: only compressed bytes cross PCIe, and none passes through a host
    copy).  A container whose blocks are not line-aligned is refused: a run of its blocks
    would not be a batch of whole lines."""

    HEADER = 32

    def __init__(self, path: str):
        from . import lz4
        self.path = str(path)
        self.size = os.path.getsize(self.path)
        self._mm = None
        self.data = np.zeros(0, dtype=np.uint8)
        if self.size:
            with open(self.path, "rb") as f:
                self._mm = mmap.mmap(f.fileno(), 0, flags=mmap.MAP_SHARED, prot=mmap.PROT_READ)
            self.data = np.frombuffer(self._mm, dtype=np.uint8)
        self.frame = lz4.is_frame(self.data[:4].tobytes())
        self.comp_bytes = 0
        self.batches = 0
        if self.frame:
            # a standard LZ4 frame (lz4 -B4 -BI, ysb_gen --lz4-frame, ysb_amd.lz4.frame_write),
            # told from the container by its magic: indexed here, measured and decoded on the GPU
            self.index, info = lz4.frame_index(self.data)
            self.directory = np.zeros((0, 2), dtype=np.uint32)
            self.raw_bytes = int(info["content_bytes"])   # (what the frames state; 0 if none does)
            return
        if self.size < self.HEADER or self.data[:8].tobytes() != lz4.FILE_MAGIC:
            raise ValueError("%s: not a compressed replay file (ysb_gen --lz4 writes one)" % self.path)
        version, flags = (int(x) for x in self.data[8:16].view(np.uint32))
        n, raw = (int(x) for x in self.data[16:32].view(np.uint64))
        if version != 1:
            raise ValueError("%s: not a compressed replay file (ysb_gen --lz4 writes one)" % self.path)
        if n > (self.size - self.HEADER) // 8:
            raise ValueError("%s: its directory is longer than the file" % self.path)
        self.directory = self.data[self.HEADER:self.HEADER + 8 * n].view(np.uint32).reshape(-1, 2)
        self.blocks_at = self.HEADER + 8 * n
        self.comp = (self.directory[:, 0] & 0x7FFFFFFF).astype(np.int64)
        self.start = np.concatenate(([0], np.cumsum(self.comp)))
        if int(self.start[-1]) != self.size - self.blocks_at or int(self.directory[:, 1].sum()) != raw:
            raise ValueError("%s: the directory does not match the file's size" % self.path)
        if not flags & lz4.FILE_LINE_ALIGNED:
            raise ValueError("%s: its blocks are not line-aligned (ysb_gen --lz4 writes them so): "
                             "a run of blocks would cut lines" % self.path)
        self.raw_bytes = raw
        self.comp_bytes = 0
        self.batches = 0

    @property
    def mapping_bytes(self) -> int:
        return (self.size + PAGE - 1) // PAGE * PAGE

    def runs(self, cap: int):
        if cap <= 0:
            raise ValueError("cap must be positive")
        if self.frame:
            # runs of consecutive blocks whose span and (blocks + 1) x 65536 both fit cap
            n, b = self.index.size, 0
            end = self.index["offset"].astype(np.int64) + (self.index["comp_bytes"] & 0x7FFFFFFF).astype(np.int64)
            while b < n:
                e, first = b, int(self.index[b]["offset"])
                while e < n and int(end[e]) - first <= cap and (e - b + 2) * 65536 <= cap:
                    e += 1
                if e == b:
                    raise ValueError("%s: block %d exceeds the slot" % (self.path, b))
                yield first, int(end[e - 1]) - first, b, e - b
                b = e
            return
        n, b = self.directory.shape[0], 0
        while b < n:
            e, comp, raw = b, 0, 0
            while e < n and comp + int(self.comp[e]) <= cap and raw + int(self.directory[e, 1]) <= cap:
                comp += int(self.comp[e])
                raw += int(self.directory[e, 1])
                e += 1
            if e == b:
                raise ValueError("%s: block %d exceeds the slot" % (self.path, b))
            yield self.blocks_at + int(self.start[b]), comp, b, e - b
            b = e

    def run(self, ctx, cap: int):
        """Every run of the container through ctx (a YsbContext), in place; returns the
        compressed bytes submitted.  At most two batches in flight."""
        ctx.host_register(self.data, self.mapping_bytes)
        try:
            slot = 0
            for off, comp, b, k in self.runs(cap):
                if self.frame:   # frame blocks end mid-line: every batch but the last leaves its tail to the next
                    ctx.submit_lz4_blocks_mapped(self.data, self.index[b:b + k], slot=slot, more=b + k < self.index.size)
                else:
                    ctx.submit_lz4_mapped(self.data, off, comp, self.directory[b:b + k], slot=slot)
                slot ^= 1
                ctx.wait(slot)
                self.comp_bytes += comp
                self.batches += 1
            ctx.sync()
        finally:
            ctx.host_unregister(self.data)
        return self.comp_bytes

    def close(self):
        self.data = np.zeros(0, dtype=np.uint8)
        self.directory = np.zeros((0, 2), dtype=np.uint32)
        if self._mm is not None:
            try:
                self._mm.close()
            except BufferError:   # a caller still holds a view of the mapping: it stays until freed
                pass
            self._mm = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class KafkaLogDataSource:
    """A partition's .log segment (or a saved fetch response) -- Kafka record batches, message
    format v2, back to back (ysb_gen --kafka, ysb_amd.kafka.write_file) --, mapped read-only:
    `runs(cap, max_records)` yields (offset into the mapping, bytes, first batch, batches) of
    runs of whole batches that fit a slot; `run(ctx, cap)` registers the mapping and submits
    every run where it lies (ysb_submit_kafka_mapped: the framed bytes cross PCIe once, the host
    reads one 61-byte header per batch).  A tail that is not a whole batch is left alone.
    codecs=("lz4",): the segment's batches may be LZ4-compressed (ysb_gen --kafka --kafka-codec lz4);
    runs are then also cut by the guaranteed bound on what they inflate to, 65536 bytes per block,
    and submitted with ysb_submit_kafka_lz4_mapped.  Without it a compressed batch is refused.
    codecs=("lz4", "snappy"): snappy batches (ysb_gen --kafka --kafka-codec snappy, either framing)
    are read too; a snappy block counts what its preamble says, and `run` tells the context
    (ysb_kafka_set_codecs; the setting stays).
    check_crc: True verifies every batch's CRC-32C on the host at index time; "device" leaves the
    data batches to the GPU (`run` turns ysb_kafka_set_crc on for its submits) and verifies on the
    host only the control batches the index skips."""

    def __init__(self, path: str, check_crc=False, codecs=()):
        from . import kafka
        if check_crc not in (False, True, "device"):
            raise ValueError("check_crc %r: False, True (the host pass) or \"device\"" % (check_crc,))
        self.crc_device = check_crc == "device"
        check_control, check_crc = self.crc_device, check_crc is True
        self.path = str(path)
        self.size = os.path.getsize(self.path)
        self._mm = None
        self.data = np.zeros(0, dtype=np.uint8)
        if self.size:
            with open(self.path, "rb") as f:
                self._mm = mmap.mmap(f.fileno(), 0, flags=mmap.MAP_SHARED, prot=mmap.PROT_READ)
            self.data = np.frombuffer(self._mm, dtype=np.uint8)
        codecs = tuple(codecs or ())
        if any(c not in ("lz4", "snappy") for c in codecs):
            raise ValueError("codecs %r: \"lz4\" and \"snappy\" are the codecs that are read" % (codecs,))
        self.lz4 = bool(codecs)          # the compressed path (ysb_submit_kafka_lz4_mapped)
        self.snappy = "snappy" in codecs
        self.frames = self.blocks = None
        if self.lz4:
            self.index, self.frames, self.blocks, self.summary = kafka.index_lz4(
                self.data, check_crc=check_crc, check_control_crc=check_control, accept_snappy=self.snappy)
        else:
            self.index, self.summary = kafka.index(self.data, check_crc=check_crc, check_control_crc=check_control)
        self.framed_bytes = 0
        self.batches = 0

    @property
    def mapping_bytes(self) -> int:
        return (self.size + PAGE - 1) // PAGE * PAGE

    def runs(self, cap: int, max_records: int):
        if cap <= 0 or max_records <= 0:
            raise ValueError("cap and max_records must be positive")
        n, b = self.index.size, 0
        start = self.index["records_off"].astype(np.int64) - 61
        end = self.index["records_off"].astype(np.int64) + self.index["records_bytes"].astype(np.int64)
        from . import kafka
        infl = kafka.inflate_bounds(self.data, self.index, self.frames, self.blocks) if self.lz4 else np.zeros(n, dtype=np.int64)
        while b < n:
            e, recs, raw = b, 0, 0
            while e < n and int(end[e]) - int(start[b]) <= cap and recs + int(self.index[e]["n_records"]) <= max_records \
                    and raw + int(infl[e]) <= cap:
                recs += int(self.index[e]["n_records"])
                raw += int(infl[e])
                e += 1
            if e == b:
                raise ValueError("%s: batch %d exceeds the slot" % (self.path, b))
            yield int(start[b]), int(end[e - 1]) - int(start[b]), b, e - b
            b = e

    def run(self, ctx, cap: int):
        """Every run of the segment through ctx (a YsbContext), in place; returns the framed
        bytes submitted.  At most two batches in flight."""
        from . import kafka
        if self.snappy:
            ctx.kafka_set_codecs(("lz4", "snappy"))
        max_bytes, max_events = ctx.slot_capacity()
        max_records = max(max_events, max_bytes // 32)
        if self.size:
            ctx.host_register(self.data, self.mapping_bytes)
        crc_before = ctx.kafka_crc_info()["mode"] if self.crc_device else None
        if self.crc_device:
            ctx.kafka_set_crc(kafka.CRC_DEVICE)
        try:
            slot = 0
            for off, nbytes, b, k in self.runs(min(cap, max_bytes), max_records):
                idx = self.index[b:b + k].copy()
                idx["records_off"] -= off
                idx["first_record"] -= idx["first_record"][0]
                if self.lz4:
                    fr = self.frames[b:b + k].copy()
                    f0 = int(fr["first_block"][0])
                    bl = self.blocks[f0:f0 + int(fr["n_blocks"].sum())].copy()
                    fr["first_block"] -= f0
                    bl["offset"] -= off
                    ctx.submit_kafka_lz4_mapped(self.data, off, nbytes, idx, fr, bl, slot=slot)
                else:
                    ctx.submit_kafka_mapped(self.data, off, nbytes, idx, slot=slot)
                slot ^= 1
                ctx.wait(slot)
                self.framed_bytes += nbytes
                self.batches += 1
            ctx.sync()
        finally:
            if self.crc_device:
                ctx.kafka_set_crc(crc_before)      # the context's setting is the caller's again
            if self.size:
                ctx.host_unregister(self.data)
        return self.framed_bytes

    def close(self):
        self.data = np.zeros(0, dtype=np.uint8)
        if self._mm is not None:
            try:
                self._mm.close()
            except BufferError:   # a caller still holds a view of the mapping: it stays until freed
                pass
            self._mm = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
