"""Per-chunk decoders of the device parquet read (K1).

read_files_batch_device uploads a file's bytes and calls decode_chunks on
the file's HIP stream; everything here launches on the current stream and
writes into the preallocated columns of a DecodeState.  Page layouts come
from native_parquet (Page / DictPage / ColumnChunkLayout).
"""

from __future__ import annotations

import sys
import time
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .logical_types import convert_torch
from .native_parquet import _decode_defs, decode_splain_pages
from .staging import _DEV_RATIO, _codec_pool, _pinned_get, _tl_decompress


@dataclass
class DecodeState:
    """What the decoders of one read share.  Worker threads append to the
    lists; every unit writes its own row range of ``out``."""
    device: object
    ext: object                        # the HIP extension module
    names: List[str]
    file_base: np.ndarray              # first output row of each file
    out: Dict[str, torch.Tensor]
    out_masks: Dict[str, torch.Tensor]
    timing: Optional[str] = None       # HS_DECODE_TIMING
    # snappy per-page status words, checked once after the sync
    statuses: List[torch.Tensor] = field(default_factory=list)
    # (name, abs row start, abs row end, dictionary values) per string
    # run — merged into one dictionary per column after the sync
    str_chunks: List[Tuple[str, int, int, List[str]]] = \
        field(default_factory=list)
    # pinned codec staging buffers, alive until the streams drain
    keepalive: List[torch.Tensor] = field(default_factory=list)


def convert_logical(col: torch.Tensor, conv) -> torch.Tensor:
    """The convert step of the device read: a decoded PHYSICAL column ->
    its engine representation (logical_types.Conv), one elementwise torch
    op on the current stream.  Runs once per annotated column after the
    decode streams have joined; un-annotated columns never reach it."""
    return convert_torch(col, conv)


def split_row_groups(chunks):
    """[(row_offset, chunks-of-one-row-group)] — layout order is
    row-group-major, so a repeated column name starts a new group."""
    groups = []
    cur: list = []
    seen = set()
    row_off = 0
    for c in chunks:
        if c.name in seen:
            groups.append((row_off, cur))
            row_off += cur[0].num_values
            cur = []
            seen = set()
        cur.append(c)
        seen.add(c.name)
    if cur:
        groups.append((row_off, cur))
    return groups


class SegmentPlan(NamedTuple):
    """Where each compressed segment of a chunk decompresses."""
    segs: List[Tuple[int, int, int]]   # (file start, file end, unc size)
    offsets: List[int]                 # scratch offset per segment + total
    dev: List[int]                     # segments for the device kernel
    host: List[int]                    # segments for the host codec pool
    identity: List[int]                # stored uncompressed: plain copies
    has_dict: bool                     # segment 0 is the dictionary page

    @property
    def page_base(self) -> List[int]:
        """Scratch offset of each data page's decompressed payload."""
        return self.offsets[1:-1] if self.has_dict else self.offsets[:-1]


def plan_segments(c, dev_ratio: float) -> SegmentPlan:
    """Latency/bandwidth split of a compressed chunk's segments (dict
    page first).  A page that actually COMPRESSED is copy-dense — a
    serial ~150-500 ns/op chain on a single wave (a 1 MB dictionary page
    of small-valued int64s measured 137 ms as 264k tiny ops,
    profiles/r2_summary.md) — so it decodes on the HOST C++ codec (~GB/s
    per worker thread) and uploads; near-incompressible snappy pages
    (comp >= ratio * unc, giant literals) stay on device where decode is
    a bandwidth-bound copy.  gzip/zstd/brotli/lz4 are host only; a V2
    is_compressed=false page is an identity copy."""
    has_dict = c.encoding == "dict_z"
    segs = []
    if has_dict:
        segs.append((c.dict_page.start, c.dict_page.end,
                     c.dict_page.unc_size))
    identity = []
    for p in c.pages:
        if not p.is_compressed:
            identity.append(len(segs))
        segs.append((p.start, p.end, p.unc_size))
    offsets = [0]
    for s in segs:
        offsets.append(offsets[-1] + s[2])
    skip = set(identity)
    if c.codec == "SNAPPY":
        dev = [i for i, s in enumerate(segs) if i not in skip
               and (s[1] - s[0]) >= dev_ratio * s[2]]
        skip.update(dev)
    else:
        dev = []
    host = [i for i in range(len(segs)) if i not in skip]
    return SegmentPlan(segs, offsets, dev, host, identity, has_dict)


def decompress_to_scratch(st: DecodeState, c, plan: SegmentPlan, buf,
                          dev_bytes):
    """Decompress every segment of ``plan`` into one device scratch
    buffer -> (scratch, {segment: host-resident decompressed bytes})."""
    segs, offsets = plan.segs, plan.offsets
    scratch = torch.empty(offsets[-1] + 4, dtype=torch.uint8,
                          device=st.device)
    for i in plan.identity:
        # torch u8 slice copy: arbitrary alignment, async on the stream
        a, _, unc = segs[i]
        scratch[offsets[i]:offsets[i] + unc] = dev_bytes[a:a + unc]
    if plan.dev:
        def t64(k):
            return torch.tensor([x[k] for x in (segs[i] for i in plan.dev)],
                                dtype=torch.int64)
        st.statuses.append(st.ext.snappy_decompress(
            dev_bytes, t64(0), t64(1), scratch,
            torch.tensor([offsets[i] for i in plan.dev],
                         dtype=torch.int64), t64(2)))
    host_bytes: Dict[int, object] = {}
    if not plan.host:
        return scratch, host_bytes
    # parquet LZ4 / LZ4_RAW pages are raw LZ4 blocks
    codec_name = ("lz4_raw" if c.codec in ("LZ4", "LZ4_RAW")
                  else c.codec.lower())
    hview = buf.numpy()
    # stage all host-decoded pages in ONE pinned buffer: the codec reads
    # the compressed page zero-copy from the read buffer, one host memcpy
    # lands it in pinned memory, and the H2D is a true async copy (a
    # per-page pageable copy_ serialized the decode stream on every page)
    hstage = _pinned_get(sum(segs[i][2] for i in plan.host))
    st.keepalive.append(hstage)
    hoffs = []
    hoff = 0
    for i in plan.host:
        hoffs.append(hoff)
        hoff += segs[i][2]

    def _stage(i, off):
        a, b, unc = segs[i]
        dec = _tl_decompress(codec_name, hview[a:b], unc)
        if len(dec) != unc:
            raise ValueError("short page")
        st.ext.host_memcpy(hstage, off, dec)
        return dec

    # fan the per-page codec calls AND the pinned staging memcpy over the
    # shared codec pool — the pyarrow codecs release the GIL, and
    # host_memcpy releases it for the copy (a numpy slice assignment held
    # it for ~GB of memcpy per read, serializing all 16 workers)
    futs = [_codec_pool().submit(_stage, i, off)
            for i, off in zip(plan.host, hoffs)]
    for i, fut, off in zip(plan.host, futs, hoffs):
        unc = segs[i][2]
        try:
            # host-decoded payloads stay available for the header/run
            # parse — it reads them WITHOUT a device round-trip (a
            # scratch D2H sync serialized every chunk on its own
            # decompression)
            host_bytes[i] = fut.result()
        except Exception:  # noqa: BLE001
            st.statuses.append(torch.ones(1, dtype=torch.int32,
                                          device=st.device))
            continue
        scratch[offsets[i]:offsets[i] + unc].copy_(
            hstage[off:off + unc], non_blocking=True)
    return scratch, host_bytes


class _ZChunk(NamedTuple):
    """A compressed chunk after decompression, as its decoders see it."""
    chunk: object
    scratch: torch.Tensor
    host_bytes: Dict[int, object]      # by segment index
    page_base: List[int]
    seg0: int                          # segment index of page 0
    dict_vals: Optional[torch.Tensor]  # numeric dictionary on device
    vals_list: Optional[List[str]]     # string dictionary on host
    has_spz: bool                      # chunk carries splain_z pages


def decode_z_chunk(st: DecodeState, c, buf, dev_bytes, written: int) -> int:
    """Compressed chunk (K1): decompress into scratch; PLAIN pages copy
    straight from scratch, dictionary-index pages parse their runs on
    host and gather through the decompressed dictionary on device.
    Returns the row cursor after the chunk."""
    t_c0 = time.perf_counter()
    plan = plan_segments(c, _DEV_RATIO)
    scratch, host_bytes = decompress_to_scratch(st, c, plan, buf, dev_bytes)
    has_spz = any(p.kind == "splain_z" for p in c.pages)
    dict_vals = vals_list = None
    if plan.has_dict and c.is_string:
        # string dictionary: small D2H of the decompressed dict page,
        # parsed to values on host; indices stay on device as the codes
        hb0 = host_bytes.get(0)
        draw = (np.frombuffer(hb0, dtype=np.uint8) if hb0 is not None
                else scratch[:c.dict_page.unc_size].cpu().numpy())
        vals_list = []
        pos = 0
        for _ in range(c.dict_page.num_values):
            ln = int(np.frombuffer(draw, "<u4", 1, pos)[0])
            pos += 4
            vals_list.append(draw[pos:pos + ln].tobytes().decode("utf-8"))
            pos += ln
        if not has_spz:
            st.str_chunks.append(
                (c.name, written,
                 written + sum(p.num_values for p in c.pages), vals_list))
        # with dictionary-overflow PLAIN pages in the chunk the
        # dictionary spans become per-run entries in the decoders
    elif plan.has_dict:
        dict_n = c.dict_page.num_values
        dict_vals = torch.empty(dict_n + 1, dtype=st.out[c.name].dtype,
                                device=st.device)
        st.ext.copy_unaligned(scratch, 0, dict_vals, 0,
                              dict_n * c.np_dtype.itemsize)
        dict_vals = dict_vals[:dict_n].contiguous()
    z = _ZChunk(c, scratch, host_bytes, plan.page_base,
                1 if plan.has_dict else 0, dict_vals, vals_list, has_spz)
    if c.name not in st.out_masks:
        end = _decode_z_fast(st, z, written, t_c0)
        if end is not None:
            return end
        # rare malformed/empty-dict page: the general per-page path
    return _decode_z_general(st, z, written)


def _fetch_page_heads(z: _ZChunk):
    """Host copy of every byte the fast path parses — whole dict_z
    payloads, else the 4-byte level-length prefix — with ONE cat + D2H
    sync per chunk for the pages not already host-resident.
    -> (bytes, per-page offset into them or -1)"""
    pieces = []
    dev_parts = []   # scratch slices still needing D2H
    dev_marks = []   # their slots in pieces
    roff = []
    cur = 0
    host_bytes, seg0 = z.host_bytes, z.seg0
    for j, page in enumerate(z.chunk.pages):
        if page.kind == "dict_z":
            ln_span = page.unc_size
        elif page.has_levels:
            ln_span = 4
        else:
            roff.append(-1)
            continue
        roff.append(cur)
        hbuf = host_bytes.get(j + seg0)
        if hbuf is not None:
            pieces.append(np.frombuffer(hbuf, dtype=np.uint8,
                                        count=ln_span))
        else:
            dev_marks.append(len(pieces))
            pieces.append(None)
            base = z.page_base[j]
            dev_parts.append(z.scratch[base:base + ln_span])
        cur += ln_span
    if dev_parts:
        dv = torch.cat(dev_parts).cpu().numpy()
        off = 0
        for m, part in zip(dev_marks, dev_parts):
            pieces[m] = dv[off:off + part.numel()]
            off += part.numel()
    hb = np.concatenate(pieces) if pieces else np.empty(0, dtype=np.uint8)
    return hb, roff


def _decode_z_fast(st: DecodeState, z: _ZChunk, written: int,
                   t_c0: float) -> Optional[int]:
    """No-null compressed chunk: all page headers (level-length prefixes,
    bit widths) are read from HOST memory and the dictionary-index runs
    of every page parse in one GIL-released C++ call per bit width (per-
    page torch slicing + a level-prefix sync per chunk serialized
    26-unit decodes on the GIL).  Returns the row cursor after the
    chunk, or None on a malformed page (nothing final written)."""
    c = z.chunk
    itemsize = c.np_dtype.itemsize
    out, copy_unaligned = st.out[c.name], st.ext.copy_unaligned
    scratch, page_base, vals_list = z.scratch, z.page_base, z.vals_list
    hb, roff = _fetch_page_heads(z)
    t_a = time.perf_counter()
    groups: Dict[int, list] = {}  # bw -> (abs_row, nv, lo, hi, bit shift)
    sp_zp = []                    # splain_z: (abs_row, nv, lo, hi)
    row = written
    run_lo = written              # dict-page run (string chunks)
    for j, page in enumerate(c.pages):
        nv = page.num_values
        base = page_base[j]
        r0 = roff[j]
        skip = 0
        if page.has_levels:
            skip = 4 + int(np.frombuffer(hb, "<u4", 1, r0)[0])
        if page.kind == "dict_z":
            bw = int(hb[r0 + skip])
            if bw <= 0 or skip + 1 >= page.unc_size:
                return None
            groups.setdefault(bw, []).append(
                (row, nv, r0 + skip + 1, r0 + page.unc_size,
                 (base - r0) * 8))
        elif page.kind == "splain_z":
            if vals_list is not None and row > run_lo:
                st.str_chunks.append((c.name, run_lo, row, vals_list))
            sp_zp.append((row, nv, base + skip, base + page.unc_size))
            run_lo = row + nv
        else:
            copy_unaligned(scratch, base + skip, out, row * itemsize,
                           nv * itemsize)
        row += nv
    if z.has_spz and vals_list is not None and row > run_lo:
        st.str_chunks.append((c.name, run_lo, row, vals_list))
    _decode_index_groups(st, z, groups, torch.from_numpy(hb))
    if sp_zp:
        _decode_splain_z_pages(st, z, sp_zp)
    if st.timing == "3":
        print(f"[hs-chunk] {c.name} pages={len(c.pages)} "
              f"pre={t_a-t_c0:.3f} fast={time.perf_counter()-t_a:.3f}",
              file=sys.stderr)
    return row


def _decode_index_groups(st: DecodeState, z: _ZChunk, groups, hb_t):
    """One run parse + rle_decode (+ gather) per bit width over all of a
    chunk's dict_z pages."""
    def t64(x):
        return torch.tensor(x, dtype=torch.int64)
    out = st.out[z.chunk.name]
    for bw, pages_g in groups.items():
        nvs = [g[1] for g in pages_g]
        outs = [0]
        for nv in nvs[:-1]:
            outs.append(outs[-1] + nv)
        drows = outs[-1] + nvs[-1]
        kind, ooff, ln_t, boff, val, _cnt = st.ext.parse_rle_runs_batch(
            hb_t, t64([g[2] for g in pages_g]), t64([g[3] for g in pages_g]),
            t64([bw] * len(pages_g)), t64(nvs), t64(outs),
            t64([g[4] for g in pages_g]))
        idx = st.ext.rle_decode(z.scratch, kind, ooff, ln_t, boff, val, bw,
                                drows)
        vals = idx if z.chunk.is_string else \
            st.ext.gather_rows(z.dict_vals, idx.to(torch.int64))
        for (abs_row, nv, _, _, _), drow in zip(pages_g, outs):
            out[abs_row:abs_row + nv] = vals[drow:drow + nv]


def _decode_splain_z_pages(st: DecodeState, z: _ZChunk, sp_zp):
    """One D2H of the decompressed byte-array payloads, one host parse +
    dict-encode, codes back up per page."""
    pb = torch.cat([z.scratch[a:b] for _, _, a, b in sp_zp]).cpu()
    ends = np.cumsum([b - a for _, _, a, b in sp_zp]).tolist()
    codes_all, spz_vals = decode_splain_pages(
        pb, [0] + ends[:-1], ends, [nv for _, nv, _, _ in sp_zp])
    name = z.chunk.name
    cpos = 0
    for abs_row, nv, _, _ in sp_zp:
        st.out[name][abs_row:abs_row + nv] = torch.from_numpy(
            np.ascontiguousarray(codes_all[cpos:cpos + nv])).to(
            st.device, non_blocking=True)
        st.str_chunks.append((name, abs_row, abs_row + nv, spz_vals))
        cpos += nv


def _fetch_levels_and_indices(z: _ZChunk, nullable: bool):
    """General path D2H: level-length prefixes of every leveled page in
    one small copy (4 bytes each), then the level bytes (nullable chunks)
    and index streams in one cat — NEVER the whole chunk (plain page
    payloads can be hundreds of MB).
    -> (lvl_skips, {(page, tag): (start in hb_all, length, abs)}, hb_all)"""
    pages = z.chunk.pages
    lvl_skips = [0] * len(pages)
    with_lvl = [j for j, p in enumerate(pages) if p.has_levels]
    if with_lvl:
        pref = torch.stack([z.scratch[z.page_base[j]:z.page_base[j] + 4]
                            for j in with_lvl]).cpu()
        for j, ln in zip(with_lvl, pref.numpy().view("<u4").ravel()):
            lvl_skips[j] = 4 + int(ln)
    regions = {}
    cat_parts = []
    cur = 0
    for j, page in enumerate(pages):
        base = z.page_base[j]
        spans = []
        if page.has_levels and nullable:
            spans.append(("lvl", base + 4, base + lvl_skips[j]))
        if page.kind == "dict_z":
            spans.append(("idx", base + lvl_skips[j],
                          base + page.unc_size))
        for tag, a, b in spans:
            regions[(j, tag)] = (cur, b - a, a)
            cat_parts.append(z.scratch[a:b])
            cur += b - a
    hb_all = torch.cat(cat_parts).cpu() if cat_parts else None
    return lvl_skips, regions, hb_all


def _decode_z_general(st: DecodeState, z: _ZChunk, written: int) -> int:
    """Per-page compressed decode: nullable chunks, and the hand-off from
    the fast path.  Unmasked dict_z pages still batch into one rle_decode
    + gather per (chunk, bit width)."""
    c, ext, scratch = z.chunk, st.ext, z.scratch
    out = st.out[c.name]
    itemsize = c.np_dtype.itemsize
    nullable = c.name in st.out_masks
    per_run = c.is_string and z.has_spz and z.vals_list is not None
    lvl_skips, regions, hb_all = _fetch_levels_and_indices(z, nullable)
    zbatch: Dict[int, dict] = {}
    for j, page in enumerate(c.pages):
        nv = page.num_values
        base = z.page_base[j]
        skip = 0
        # V2 pages carry their mask from the layout parse (levels live
        # uncompressed in the file); V1 pages decode the level prefix
        # from the decompressed payload here
        pmask = c.page_masks[j]
        if pmask is None and page.has_levels:
            skip = lvl_skips[j]
            if nullable:
                s0, rln, _ = regions[(j, "lvl")]
                pmask = _decode_defs(hb_all[s0:s0 + rln].numpy().tobytes(),
                                     0, skip - 4, nv,
                                     getattr(c, "max_def", 1))
        n_valid = int(pmask.sum()) if pmask is not None else nv
        if page.kind == "dict_z":
            s0, rln, absbase = regions[(j, "idx")]
            bw = int(hb_all[s0])
            runs = list(ext.parse_rle_runs(hb_all, s0 + 1, s0 + rln, bw,
                                           n_valid))
            # bit-offsets: cat-local -> scratch coordinates
            runs[3] = runs[3] + (absbase - s0) * 8
            if pmask is None:
                lst = zbatch.setdefault(
                    bw, {"runs": [], "rows": 0, "pages": []})
                runs[1] = runs[1] + lst["rows"]
                lst["runs"].append(runs)
                lst["pages"].append((written, nv, lst["rows"]))
                lst["rows"] += nv
                written += nv
                continue
            idx = ext.rle_decode(scratch, *runs, bw, n_valid)
            vals = idx if c.is_string else ext.gather_rows(
                z.dict_vals, idx.to(torch.int64))
            if per_run:
                st.str_chunks.append((c.name, written, written + nv,
                                      z.vals_list))
        elif page.kind == "splain_z":
            # decompressed PLAIN byte-array payload: D2H, host parse +
            # dict-encode, codes back up
            pb = scratch[base + skip:base + page.unc_size].cpu()
            codes_np, pvals = decode_splain_pages(
                pb, [0], [int(pb.numel())], [n_valid])
            vals = torch.from_numpy(
                np.ascontiguousarray(codes_np)).to(st.device)
            st.str_chunks.append((c.name, written, written + nv, pvals))
        elif pmask is None:
            ext.copy_unaligned(scratch, base + skip, out,
                               written * itemsize, nv * itemsize)
            written += nv
            continue
        else:
            vals = torch.empty(n_valid + 1, dtype=out.dtype,
                               device=st.device)
            ext.copy_unaligned(scratch, base + skip, vals, 0,
                               n_valid * itemsize)
            vals = vals[:n_valid]
        if pmask is None:
            out[written:written + nv] = vals
        else:
            mask_dev = torch.from_numpy(pmask).to(st.device)
            dst = out[written:written + nv]
            dst.zero_()
            dst[mask_dev] = vals
            st.out_masks[c.name][written:written + nv] = mask_dev
        written += nv
    for bw, lst in zbatch.items():
        cat = [torch.cat([r[k] for r in lst["runs"]]) for k in range(5)]
        idx = ext.rle_decode(scratch, *cat, bw, lst["rows"])
        vals = idx if c.is_string else ext.gather_rows(
            z.dict_vals, idx.to(torch.int64))
        for woff, nv, rbase in lst["pages"]:
            out[woff:woff + nv] = vals[rbase:rbase + nv]
            if per_run:
                st.str_chunks.append((c.name, woff, woff + nv,
                                      z.vals_list))
    return written


class _PlainDicts(NamedTuple):
    """Dictionaries of an uncompressed chunk, prepared once per chunk."""
    dict_vals: Optional[torch.Tensor]  # numeric dictionary on device
    chunk_dict: Optional[List[str]]    # string dictionary page values
    sp_codes: Dict[int, np.ndarray]    # page -> codes of a splain page
    sp_vals: Optional[List[str]]       # the dictionary those codes use


def _plain_dicts(st: DecodeState, c, buf, dev_bytes) -> _PlainDicts:
    if c.is_string:
        # string chunk (K1): indices ARE the column (int32 codes into the
        # host-parsed dictionary) — no value gather; per-run str_chunks
        # spans merge after the sync.  PLAIN byte-array pages (whole-
        # chunk PLAIN, or the writer's mid-chunk dictionary overflow)
        # parse host-side in one GIL-released call and dictionary-encode
        # per chunk; their codes upload directly.
        chunk_dict = c.dict_values(buf.numpy()) if c.dict_page else None
        sp = [j for j, p in enumerate(c.pages) if p.kind == "splain"]
        sp_codes: Dict[int, np.ndarray] = {}
        sp_vals = None
        if sp:
            counts = [(int(c.page_masks[j].sum())
                       if c.page_masks[j] is not None
                       else c.pages[j].num_values) for j in sp]
            all_codes, sp_vals = decode_splain_pages(
                buf, [c.pages[j].start for j in sp],
                [c.pages[j].end for j in sp], counts)
            cur = 0
            for j, n_valid in zip(sp, counts):
                sp_codes[j] = all_codes[cur:cur + n_valid]
                cur += n_valid
        return _PlainDicts(None, chunk_dict, sp_codes, sp_vals)
    if c.encoding != "dict":
        return _PlainDicts(None, None, {}, None)
    # K1 dictionary path: decode the dictionary page once; pages gather
    # through it (a chunk can also carry PLAIN pages — the writer's
    # mid-chunk dictionary-overflow fallback)
    dict_n = c.dict_page.num_values
    dict_vals = torch.empty(dict_n + 1,  # +1 slack for the 4B-overread
                            dtype=st.out[c.name].dtype, device=st.device)
    st.ext.copy_unaligned(dev_bytes, c.dict_page.start, dict_vals, 0,
                          dict_n * c.np_dtype.itemsize)
    return _PlainDicts(dict_vals[:dict_n].contiguous(), None, {}, None)


def _upload_codes(st: DecodeState, codes) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(codes)).to(
        st.device, non_blocking=True)


def decode_plain_chunk(st: DecodeState, c, buf, dev_bytes,
                       written: int) -> int:
    """Uncompressed chunk without nulls: every page decodes straight
    into its rows.  Returns the row cursor after the chunk."""
    ext, out = st.ext, st.out[c.name]
    itemsize = c.np_dtype.itemsize
    d = _plain_dicts(st, c, buf, dev_bytes)
    run_lo = written  # current dict-page run (string chunks)
    for j, page in enumerate(c.pages):
        nv = page.num_values
        if page.kind == "dict":
            runs = ext.parse_rle_runs(buf, page.start, page.end,
                                      page.bit_width, nv)
            idx = ext.rle_decode(dev_bytes, *runs, page.bit_width, nv)
            out[written:written + nv] = idx if c.is_string else \
                ext.gather_rows(d.dict_vals, idx.to(torch.int64))
        elif page.kind == "splain":
            if written > run_lo:
                st.str_chunks.append((c.name, run_lo, written,
                                      d.chunk_dict))
            out[written:written + nv] = _upload_codes(st, d.sp_codes[j])
            st.str_chunks.append((c.name, written, written + nv,
                                  d.sp_vals))
            run_lo = written + nv
        else:
            ext.copy_unaligned(dev_bytes, page.start, out,
                               written * itemsize, nv * itemsize)
        written += nv
    if c.is_string and written > run_lo:
        st.str_chunks.append((c.name, run_lo, written, d.chunk_dict))
    return written


def decode_nullable_chunk(st: DecodeState, c, buf, dev_bytes,
                          written: int) -> int:
    """Uncompressed chunk with nulls: decode every page's compacted
    values into ONE temp, then a single chunk-wide scatter (per-page
    boolean indexing costs a kernel pair per page — thousands of launches
    on multi-page files).  Returns the row cursor after the chunk."""
    ext, out = st.ext, st.out[c.name]
    itemsize = c.np_dtype.itemsize
    d = _plain_dicts(st, c, buf, dev_bytes)
    n_rows = sum(p.num_values for p in c.pages)
    valid_counts = [int(m.sum()) if m is not None else p.num_values
                    for p, m in zip(c.pages, c.page_masks)]
    total_valid = sum(valid_counts)
    tmp = torch.empty(total_valid + 1, dtype=out.dtype, device=st.device)
    cur = 0
    row_pos = run_lo = written
    for j, (page, n_valid) in enumerate(zip(c.pages, valid_counts)):
        if page.kind == "dict":
            runs = ext.parse_rle_runs(buf, page.start, page.end,
                                      page.bit_width, n_valid)
            idx = ext.rle_decode(dev_bytes, *runs, page.bit_width, n_valid)
            tmp[cur:cur + n_valid] = idx if c.is_string else \
                ext.gather_rows(d.dict_vals, idx.to(torch.int64))
        elif page.kind == "splain":
            if row_pos > run_lo:
                st.str_chunks.append((c.name, run_lo, row_pos,
                                      d.chunk_dict))
            tmp[cur:cur + n_valid] = _upload_codes(st, d.sp_codes[j])
            st.str_chunks.append((c.name, row_pos,
                                  row_pos + page.num_values, d.sp_vals))
            run_lo = row_pos + page.num_values
        else:
            ext.copy_unaligned(dev_bytes, page.start, tmp, cur * itemsize,
                               n_valid * itemsize)
        row_pos += page.num_values
        cur += n_valid
    if c.is_string and row_pos > run_lo:
        st.str_chunks.append((c.name, run_lo, row_pos, d.chunk_dict))
    chunk_mask = np.concatenate([
        m if m is not None else np.ones(p.num_values, dtype=bool)
        for p, m in zip(c.pages, c.page_masks)])
    mask_dev = torch.from_numpy(chunk_mask).to(st.device)
    dst = out[written:written + n_rows]
    dst.zero_()
    dst[mask_dev] = tmp[:total_valid]
    st.out_masks[c.name][written:written + n_rows] = mask_dev
    return written + n_rows


def decode_chunks(st: DecodeState, file_index: int, buf, dev_bytes, chunks,
                  row_off: int) -> None:
    """Decode ``chunks`` (one file, or one row group of it starting at
    file row ``row_off``) on the current stream.  ``buf`` is the pinned
    host copy of the file and ``dev_bytes`` its device copy; the caller
    keeps both alive until the stream drains."""
    cursors = {n: int(st.file_base[file_index]) + row_off
               for n in st.names}
    for c in chunks:
        if c.encoding in ("plain_z", "dict_z", "splain_z"):
            decode = decode_z_chunk
        elif c.has_nulls:
            decode = decode_nullable_chunk
        else:
            decode = decode_plain_chunk
        cursors[c.name] = decode(st, c, buf, dev_bytes, cursors[c.name])
