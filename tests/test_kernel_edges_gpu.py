"""Kernel-edge tests: the HIP code paths that large uniform-random inputs
never reach — int64 radix payloads and the 512-bin digit, multi-block
scans, hand-built snappy and RLE pages, masks and small dtypes in the
hash, ties in the run merge, and the small kernels at their edges.

Every comparison is bit-exact against ``cpu_ref`` or the numpy oracles
of kernel_edge_common.py (validated on the CPU by
test_kernel_edge_builders.py).

Run on a GPU box: python -m pytest tests/test_kernel_edges_gpu.py -m gpu -q
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import hyperspace_amd.ops as ops
from hyperspace_amd.ops import cpu_ref, native

import kernel_edge_common as kc

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -2**63, 2**63 - 1


@pytest.fixture(scope="module", autouse=True)
def _require_native():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert native.available(), "HIP extension must load on a GPU box"


def _ext():
    return native.ext()


def _norm(v):
    return int(cpu_ref.normalize_key(torch.tensor([v]))[0])


# ---------------------------------------------------------------------------
# Radix sort
# ---------------------------------------------------------------------------

def _sort_and_compare(keys, payload):
    ck, cp = cpu_ref.stable_sort_u64(keys, payload)
    gk, gp = _ext().radix_sort_pairs(keys.cuda(), payload.cuda())
    assert gp.dtype == torch.int64
    assert torch.equal(ck, gk.cpu())
    assert torch.equal(cp, gp.cpu())
    return gk.cpu(), gp.cpu()


def _payload(kind, n):
    a = torch.arange(n, dtype=torch.int64)
    return {"i32": a, "neg": a - n // 2, "big": a + 2**40}[kind]


@pytest.mark.parametrize("keys_kind", ["full", "four"])
@pytest.mark.parametrize("payload_kind", ["neg", "big"])
@pytest.mark.parametrize("n", [2, 1023, 1024, 1025, 2049, 70_001])
def test_radix_sort_int64_payload(n, payload_kind, keys_kind):
    """Payloads outside [0, INT32_MAX) take the i64 scatter: the payload
    round-trips the u64 staging buffer and the i64 ping-pong buffers.
    Keys from [0, 4) put one digit on every lane of whole waves."""
    rng = np.random.default_rng(n)
    if keys_kind == "full":
        keys = kc.as_i64(rng.integers(0, kc.U64, n, dtype=np.uint64,
                                      endpoint=True))
    else:
        keys = torch.from_numpy(rng.integers(0, 4, n, dtype=np.int64))
    _sort_and_compare(keys, _payload(payload_kind, n))


def test_radix_sort_int64_payload_max_blocks():
    """One tile past RS_MAX_BLOCKS * 1024 keys: the block count saturates
    and blocks own more than one tile."""
    n = 2048 * 1024 + 1025
    rng = np.random.default_rng(9)
    keys = kc.as_i64(rng.integers(0, kc.U64, n, dtype=np.uint64,
                                  endpoint=True))
    _sort_and_compare(keys, _payload("neg", n))


@pytest.mark.parametrize("payload_kind", ["i32", "big"])
@pytest.mark.parametrize("n", [1025, 5000])
@pytest.mark.parametrize("shape", kc.RADIX_SHAPES)
def test_radix_sort_key_shapes(shape, n, payload_kind):
    keys = kc.radix_keys(shape, n)
    payload = _payload(payload_kind, n)
    gk, gp = _sort_and_compare(keys, payload)
    if shape == "all_equal":   # zero passes: output is the input
        assert torch.equal(gk, keys) and torch.equal(gp, payload)


def test_radix_sort_plan_default_is_byte_passes():
    """radix_sort_plan returns what the sort runs: in the default
    environment byte digits, ascending, each varying bit covered once."""
    assert os.environ.get("HS_RS_9BIT") != "1"
    ext = _ext()
    masks = [kc.varying_mask(kc.radix_keys(s, n))
             for s in kc.RADIX_SHAPES for n in (1025, 5000)]
    masks += [0, 1, 1 << 63, (1 << 26) - 1, 0x1FF00, (1 << 18) - 1, kc.U64,
              0x0100_0000_0000_0080]
    for mask in masks:
        radix, shifts = ext.radix_sort_plan(mask)
        assert radix == 256, hex(mask)
        shifts = list(shifts)
        kc.check_plan_covers(mask, radix, shifts)
        assert shifts == [s for s in range(0, 64, 8) if (mask >> s) & 0xFF]
    assert list(ext.radix_sort_plan(0)[1]) == []


def test_radix_sort_512_bin_path():
    """The 9-bit digit (u16 LDS counters, two digits per thread, 10-bit
    ballot) only runs in a process started with HS_RS_9BIT=1: a fresh
    child asserts the plan says 512 there and sorts the nine-bit planner's
    key ranges at both payload widths against cpu_ref."""
    env = dict(os.environ, HS_RS_9BIT="1")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                         "kernel_edge_nine_bit_child.py")
    cmd = [sys.executable]
    if sys.flags.no_user_site:
        cmd.append("-s")
    try:
        r = subprocess.run(cmd + [child], env=env, timeout=240,
                           capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        pytest.exit("512-bin radix child timed out: nothing more may "
                    "start on the GPU in this run", returncode=1)
    if r.returncode in (134, 139, 124, 137) or r.returncode < 0:
        pytest.exit(f"512-bin radix child died with status {r.returncode}: "
                    "nothing more may start on the GPU in this run\n"
                    + r.stdout[-2000:] + r.stderr[-4000:], returncode=1)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "12 sorts matched" in r.stdout


# ---------------------------------------------------------------------------
# Exclusive scan
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", kc.scan_inputs(), ids=lambda c: c[0])
def test_exclusive_scan(case):
    """More than 256 elements reach blockIdx > 0, the block-total scan
    with nb > 1 and the non-zero base; more than 524,288 reach
    per_block > 256."""
    _, x = case
    exp_out, exp_total = kc.exclusive_scan_ref(x)
    out, total = _ext().exclusive_scan(torch.from_numpy(x).cuda())
    assert total.shape == (1,) and total.is_cuda
    assert int(total.cpu()[0]) == exp_total
    assert np.array_equal(out.cpu().numpy(), exp_out)


def test_exclusive_scan_empty():
    out, total = _ext().exclusive_scan(
        torch.empty(0, dtype=torch.int64, device="cuda"))
    assert out.numel() == 0 and int(total.cpu()[0]) == 0


# ---------------------------------------------------------------------------
# Snappy kernel
# ---------------------------------------------------------------------------

FILL = 0xAA


def _prefill(n, seed):
    """Seeded random bytes for a destination buffer: a kernel that leaves
    a byte unwritten, or copies from a byte it should not have read,
    shows up as a mismatch whatever the page's own bytes are."""
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.fixture(scope="module")
def snappy_valid_run(_require_native):
    """All valid hand-built pages in ONE launch; dst is pre-filled with
    known bytes so those outside the pages' outputs must come back
    untouched."""
    pages = []
    for p in kc.snappy_valid_pages():
        stream, ref = kc.snappy_stream(p["ops"])
        pages.append(dict(p, stream=stream + p["trailing"], ref=ref,
                          dst_len=len(ref)))
    blob, so, se, do, total = kc.snappy_layout(pages)
    src = torch.frombuffer(bytearray(blob + bytes(4)),
                           dtype=torch.uint8).cuda()
    before = _prefill(total + 4, 90)
    dst = torch.from_numpy(before).cuda()
    st = _ext().snappy_decompress(
        src, torch.tensor(so), torch.tensor(se), dst, torch.tensor(do),
        torch.tensor([p["dst_len"] for p in pages]))
    torch.cuda.synchronize()
    return pages, do, st.cpu().numpy(), dst.cpu().numpy(), before


@pytest.mark.parametrize("idx", range(len(kc.snappy_valid_pages())),
                         ids=[p["name"] for p in kc.snappy_valid_pages()])
def test_snappy_hand_built_page(snappy_valid_run, idx):
    pages, do, st, dst, _ = snappy_valid_run
    p = pages[idx]
    assert st[idx] == 0, p["name"]
    got = dst[do[idx]:do[idx] + p["dst_len"]].tobytes()
    if got != p["ref"]:
        bad = next(i for i in range(len(got)) if got[i] != p["ref"][i])
        pytest.fail(f"{p['name']}: first differing output byte {bad} of "
                    f"{len(got)}")


def test_snappy_writes_stay_inside_pages(snappy_valid_run):
    pages, do, st, dst, before = snappy_valid_run
    covered = np.zeros(dst.size, dtype=bool)
    for p, d in zip(pages, do):
        covered[d:d + p["dst_len"]] = True
    assert not covered[-4:].any()
    assert np.array_equal(dst[~covered], before[~covered])


def test_snappy_malformed_pages_exact_status():
    bad = kc.snappy_malformed_pages()
    pages = [dict(stream=s, dst_len=n) for _, s, n, _ in bad]
    blob, so, se, do, total = kc.snappy_layout(pages)
    src = torch.frombuffer(bytearray(blob + bytes(4)),
                           dtype=torch.uint8).cuda()
    dst = torch.full((total + 4,), FILL, dtype=torch.uint8, device="cuda")
    st = _ext().snappy_decompress(
        src, torch.tensor(so), torch.tensor(se), dst, torch.tensor(do),
        torch.tensor([p["dst_len"] for p in pages]))
    torch.cuda.synchronize()
    got = dict(zip([b[0] for b in bad], st.cpu().tolist()))
    assert got == {b[0]: b[3] for b in bad}


# ---------------------------------------------------------------------------
# RLE decode and unaligned copy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("bw", kc.RLE_BIT_WIDTHS)
def test_rle_decode_bit_width(bw):
    """Every bit width 1..32 through parse_rle_runs + rle_decode.  A
    value spans five source bytes once (bit & 7) + bw > 32; runs start
    on byte boundaries, so that happens at bw 27, 29, 30 and 31."""
    ext = _ext()
    data, vals = kc.rle_encode(kc.rle_case(bw), bw)
    start = bw % 5                      # vary the stream's byte position
    host = torch.frombuffer(bytearray(bytes(start) + data + bytes(4)),
                            dtype=torch.uint8)
    runs = ext.parse_rle_runs(host, start, start + len(data), bw, vals.size)
    idx = ext.rle_decode(host.cuda(), *runs, bw, vals.size)
    assert idx.dtype == torch.int32
    got = idx.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, vals), np.flatnonzero(got != vals)[:8]


@pytest.mark.parametrize("bw", [13, 27])
def test_rle_decode_multi_page_batch(bw):
    """parse_rle_runs_batch with non-zero out_shifts and bit_shifts: the
    pages sit at different offsets in the host and device buffers."""
    ext = _ext()
    enc = [kc.rle_encode(kc.rle_case(bw, seed=s), bw) for s in (1, 2, 3)]
    host, dev = bytearray(), bytearray()
    starts, ends, bit_shifts = [], [], []
    for (data, _), hgap, dgap in zip(enc, (5, 3, 0), (11, 2, 9)):
        host += bytes([0x55]) * hgap
        dev += bytes([0x33]) * dgap
        starts.append(len(host))
        bit_shifts.append((len(dev) - len(host)) * 8)
        host += data
        dev += data
        ends.append(len(host))
    dev += bytes(4)
    nvs = [v.size for _, v in enc]
    out_shifts = [0, nvs[0], nvs[0] + nvs[1]]
    t64 = lambda a: torch.tensor(a, dtype=torch.int64)  # noqa: E731
    kind, ooff, ln, boff, val, counts = ext.parse_rle_runs_batch(
        torch.frombuffer(host, dtype=torch.uint8), t64(starts), t64(ends),
        t64([bw] * 3), t64(nvs), t64(out_shifts), t64(bit_shifts))
    assert counts.tolist() == [7, 7, 7]
    idx = ext.rle_decode(torch.frombuffer(dev, dtype=torch.uint8).cuda(),
                         kind, ooff, ln, boff, val, bw, sum(nvs))
    exp = np.concatenate([v for _, v in enc])
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), exp)


@pytest.mark.parametrize("nbytes", [4, 1020, 1024, 1028, 4096 * 4 + 4])
def test_copy_unaligned_source_residues(nbytes):
    ext = _ext()
    rng = np.random.default_rng(nbytes)
    for src_off in (0, 1, 2, 3, 8, 13, 102, 7 + 4 * 25):
        src = rng.integers(0, 256, src_off + nbytes + 4, dtype=np.uint8)
        dst_off = 12
        dst = torch.full((dst_off + nbytes + 8,), FILL, dtype=torch.uint8,
                         device="cuda")
        ext.copy_unaligned(torch.from_numpy(src).cuda(), src_off, dst,
                           dst_off, nbytes)
        exp = np.full(dst_off + nbytes + 8, FILL, dtype=np.uint8)
        exp[dst_off:dst_off + nbytes] = kc.copy_unaligned_ref(
            src, src_off, nbytes)
        assert np.array_equal(dst.cpu().numpy(), exp), (src_off, nbytes)


# ---------------------------------------------------------------------------
# Murmur3 and normalize_key
# ---------------------------------------------------------------------------

def _mask_sets(n, n_cols, rng):
    some = [torch.from_numpy(rng.integers(0, 2, n).astype(bool))
            for _ in range(n_cols)]
    none_valid = torch.zeros(n, dtype=torch.bool)
    if n_cols == 1:
        return [[some[0]], [none_valid]]
    return [[some[0], None], [None, some[1]], [some[0], some[1]],
            [none_valid, none_valid]]


@pytest.mark.parametrize("n_cols", [1, 2])
def test_murmur3_bucket_validity_masks(n_cols):
    """A null key leaves the running hash unchanged: the seed for the
    first column, the previous column's hash after it."""
    rng = np.random.default_rng(40 + n_cols)
    for n in (1, 63, 64, 65, 1000):
        keys = [torch.from_numpy(rng.integers(-2**62, 2**62, n,
                                              dtype=np.int64)),
                torch.from_numpy(rng.integers(-100, 100, n)
                                 .astype(np.int32))][:n_cols]
        for masks in _mask_sets(n, n_cols, rng):
            for nb in (1, 7, 200):
                cpu = cpu_ref.murmur3_bucket(keys, nb, masks)
                gpu = ops.murmur3_bucket(
                    [k.cuda() for k in keys], nb,
                    [m.cuda() if m is not None else None for m in masks])
                assert gpu.dtype == torch.int32
                assert torch.equal(cpu, gpu.cpu()), (n, nb)
        if n_cols == 1:   # all-null single key lands in pmod(42, nb)
            got = ops.murmur3_bucket(
                [keys[0].cuda()], 200,
                [torch.zeros(n, dtype=torch.bool).cuda()]).cpu()
            assert (got == 42).all()


def _hash_columns():
    rng = np.random.default_rng(50)
    n = 1000
    f32 = np.resize(kc.float_specials(np.float32), n)
    f64 = np.resize(kc.float_specials(np.float64), n)
    return {
        "int16": torch.from_numpy(
            rng.integers(-2**15, 2**15, n).astype(np.int16)),
        "int8": torch.from_numpy(
            rng.integers(-128, 128, n).astype(np.int8)),
        "bool": torch.from_numpy(rng.integers(0, 2, n).astype(bool)),
        "float32": torch.from_numpy(f32.copy()),
        "float64": torch.from_numpy(f64.copy()),
    }


@pytest.mark.parametrize("name", ["int16", "int8", "bool", "float32",
                                  "float64"])
def test_murmur3_bucket_small_and_float_dtypes(name):
    col = _hash_columns()[name]
    if name == "int16":
        col[:2] = torch.tensor([-2**15, 2**15 - 1], dtype=torch.int16)
    if name == "int8":
        col[:2] = torch.tensor([-128, 127], dtype=torch.int8)
    lead = torch.arange(col.numel(), dtype=torch.int64) - 500
    for keys in ([col], [lead, col], [col, lead]):
        for nb in (7, 200):
            cpu = cpu_ref.murmur3_bucket(keys, nb)
            gpu = ops.murmur3_bucket([k.cuda() for k in keys], nb).cpu()
            assert torch.equal(cpu, gpu), (name, len(keys), nb)


@pytest.mark.parametrize("name", ["int16", "int8", "bool", "float32",
                                  "float64"])
def test_normalize_key_small_ints_and_special_floats(name):
    if name.startswith("float"):
        vals = kc.float_specials(np.dtype(name).type)
        col = torch.from_numpy(
            vals[np.random.default_rng(3).permutation(vals.size)])
    else:
        col = _hash_columns()[name]
        if name == "int16":
            col[:3] = torch.tensor([-2**15, 2**15 - 1, 0],
                                   dtype=torch.int16)
        if name == "int8":
            col[:3] = torch.tensor([-128, 127, 0], dtype=torch.int8)
    cpu = cpu_ref.normalize_key(col)
    gpu = ops.normalize_key(col.cuda()).cpu()
    assert torch.equal(cpu, gpu), name


# ---------------------------------------------------------------------------
# Merge permutation, range select
# ---------------------------------------------------------------------------

def test_run_merge_perm_ties():
    """Keys from [0, 5): A and B runs tie all the time, so the A-row
    lower_bound / B-row upper_bound rule decides nearly every position."""
    rng = np.random.default_rng(60)
    seg, split, parts = [0], [], []
    for na, nb in [(300, 300), (0, 7), (7, 0), (1, 1), (2000, 3)]:
        parts += [np.sort(rng.integers(0, 5, na)),
                  np.sort(rng.integers(0, 5, nb))]
        split.append(seg[-1] + na)
        seg.append(seg[-1] + na + nb)
    raw = np.concatenate(parts).astype(np.int64)
    raw[seg[3]:seg[4]] = 2          # the (1, 1) segment is a tie
    keys = cpu_ref.normalize_key(torch.from_numpy(raw))
    seg_t, split_t = torch.tensor(seg), torch.tensor(split)
    cpu = cpu_ref.run_merge_perm(keys, seg_t, split_t)
    perm = ops.run_merge_perm(keys.cuda(), seg_t, split_t).cpu()
    assert torch.equal(cpu, perm)
    p = perm.numpy()
    assert np.array_equal(np.sort(p), np.arange(raw.size))   # a permutation
    for s in range(len(split)):
        ps = p[seg[s]:seg[s + 1]]
        assert ((ps >= seg[s]) & (ps < seg[s + 1])).all()
        merged = raw[ps]
        assert (np.diff(merged) >= 0).all()
        # equal keys: all A rows (index < split) before all B rows, each
        # run in its own order — so indices ascend within a key
        same = np.diff(merged) == 0
        assert (np.diff(ps)[same] > 0).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_select_range_edges(n):
    rng = np.random.default_rng(n)
    keys = cpu_ref.normalize_key(
        torch.from_numpy(rng.integers(-3, 4, n, dtype=np.int64)))
    if n >= 3:
        keys[0], keys[-1] = 0, -1        # u64 min and max
    dkeys = keys.cuda()
    ranges = {
        "lo_eq_hi": (_norm(0), _norm(0)),
        "inverted": (_norm(2), _norm(-2)),
        "full": (0, -1),
        "all_inner": (_norm(-3), _norm(3)),
        "none": (_norm(10), _norm(20)),
        "some": (_norm(-1), _norm(2)),
    }
    for name, (lo, hi) in ranges.items():
        for li in (True, False):
            for hi_incl in (True, False):
                cpu = cpu_ref.select_range_u64(keys, lo, hi, li, hi_incl)
                gpu = ops.select_range_u64(dkeys, lo, hi, li, hi_incl).cpu()
                assert torch.equal(cpu, gpu), (name, n, li, hi_incl)
                if name == "inverted" or name == "none":
                    assert gpu.numel() == 0
    if n >= 3:   # closed full range selects every row
        assert ops.select_range_u64(dkeys, 0, -1, True, True).numel() == n


# ---------------------------------------------------------------------------
# Bloom, z-order, gather, isin, min/max
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("m_bits", [64, 1000, 1_000_003])
def test_bloom_sizes_and_hash_counts(m_bits, k):
    rng = np.random.default_rng(m_bits + k)
    n_build = 6 if m_bits == 64 else 3000
    vals = torch.from_numpy(rng.integers(-10**12, 10**12, n_build,
                                         dtype=np.int64))
    vals[:3] = torch.tensor([-1, I64_MIN, I64_MAX])
    cpu_words = cpu_ref.bloom_build(vals, m_bits, k)
    gpu_words = ops.bloom_build(vals.cuda(), m_bits, k)
    assert torch.equal(cpu_words, gpu_words.cpu())
    probe = torch.cat([vals, torch.from_numpy(rng.integers(
        -10**12, 10**12, 3000, dtype=np.int64))])
    cpu_hit = cpu_ref.bloom_probe(probe, cpu_words, m_bits, k)
    gpu_hit = ops.bloom_probe(probe.cuda(), gpu_words, m_bits, k).cpu()
    assert torch.equal(cpu_hit, gpu_hit)
    assert gpu_hit[:n_build].all()


@pytest.mark.parametrize("n_vals", [1, 7])
@pytest.mark.parametrize("n_filters", [1, 3, 130])
def test_bloom_probe_many(n_filters, n_vals):
    m_bits, k = 1000, 3
    rng = np.random.default_rng(10 * n_filters + n_vals)
    vals = torch.from_numpy(rng.integers(-10**9, 10**9, n_vals,
                                         dtype=np.int64))
    words_per = (m_bits + 63) // 64
    filters = [cpu_ref.bloom_build(vals[-1:], m_bits, k)]  # last value only
    if n_filters > 1:
        filters.append(torch.zeros(words_per, dtype=torch.int64))  # no hit
    while len(filters) < n_filters:
        members = torch.from_numpy(rng.integers(-10**9, 10**9, 40,
                                                dtype=np.int64))
        if len(filters) % 3 == 0:
            members[0] = vals[int(rng.integers(0, n_vals))]
        filters.append(cpu_ref.bloom_build(members, m_bits, k))
    words = torch.stack(filters)
    exp = kc.bloom_probe_many_ref(vals, words, m_bits, k)
    got = ops.bloom_probe_many(vals.cuda(), words.cuda(), m_bits, k).cpu()
    assert got.dtype == torch.bool and torch.equal(exp, got)
    assert bool(got[0])
    if n_filters > 1:
        assert not bool(got[1])
    if n_filters == 130:
        assert 0 < int(got.sum()) < n_filters


@pytest.mark.parametrize("n_cols,bits", [(1, 64), (3, 21), (4, 16), (8, 8),
                                         (2, 1), (5, 0)])
def test_zorder_column_counts(n_cols, bits):
    rng = np.random.default_rng(n_cols * 100 + bits)
    cols = []
    for _ in range(n_cols):
        c = kc.as_i64(rng.integers(0, kc.U64, 1000, dtype=np.uint64,
                                   endpoint=True))
        c[:3] = torch.tensor([0, -1, I64_MIN])
        cols.append(c)
    cpu = cpu_ref.zorder_key(cols, bits)
    gpu = ops.zorder_key([c.cuda() for c in cols], bits).cpu()
    assert torch.equal(cpu, gpu)
    if bits == 0:
        assert not gpu.any()
    if n_cols == 1:
        assert torch.equal(gpu, cols[0])


@pytest.mark.parametrize("name", ["int16", "int8", "bool"])
def test_gather_rows_narrow_dtypes(name):
    vals = _hash_columns()[name]
    rng = np.random.default_rng(70)
    idx = torch.from_numpy(np.concatenate([
        rng.integers(0, vals.numel(), 700), np.full(300, 999),
        np.zeros(29, dtype=np.int64)]).astype(np.int64))
    got = ops.gather_rows(vals.cuda(), idx.cuda()).cpu()
    assert got.dtype == vals.dtype and torch.equal(vals[idx], got)
    empty = ops.gather_rows(vals.cuda(),
                            torch.empty(0, dtype=torch.int64, device="cuda"))
    assert empty.numel() == 0 and empty.dtype == vals.dtype


def test_isin_sorted_extremes():
    vals = torch.tensor([I64_MIN, I64_MIN + 1, -1, 0, 5, I64_MAX - 1,
                         I64_MAX], dtype=torch.int64)
    for s in (torch.tensor([5]), torch.tensor([I64_MIN]),
              torch.tensor([I64_MAX]),
              torch.tensor([I64_MIN, 0, I64_MAX])):
        for v in (vals, vals[:1], vals[-1:], vals[4:5]):   # n = 1 too
            cpu = cpu_ref.isin_sorted(v, s)
            gpu = ops.isin_sorted(v.cuda(), s.cuda()).cpu()
            assert torch.equal(cpu, gpu), (s.tolist(), v.tolist())


def test_segmented_minmax_many_segments():
    """5000 segments > the 4096-block grid: blocks stride over segments;
    lengths 0, 1, 257 and 600 mix empty, single-thread and multi-round
    reductions; the extreme values equal the reduction identities."""
    rng = np.random.default_rng(80)
    lens = np.resize(np.array([0, 1, 257, 600, 1, 0, 600, 257]), 5000)
    lens[-3:] = 0                                  # trailing empties
    seg = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    vals = rng.integers(I64_MIN, I64_MAX, int(seg[-1]), dtype=np.int64,
                        endpoint=True)
    vals[rng.integers(0, vals.size, 400)] = I64_MIN
    vals[rng.integers(0, vals.size, 400)] = I64_MAX
    singles = seg[:-1][lens == 1]
    vals[singles[0]], vals[singles[1]] = I64_MAX, I64_MIN
    vals_t, seg_t = torch.from_numpy(vals), torch.from_numpy(seg)
    cmin, cmax = cpu_ref.segmented_minmax(vals_t, seg_t)
    gmin, gmax = ops.segmented_minmax(vals_t.cuda(), seg_t)
    assert torch.equal(cmin, gmin.cpu())
    assert torch.equal(cmax, gmax.cpu())


# ---------------------------------------------------------------------------
# Argument guards of the binding
# ---------------------------------------------------------------------------

def test_binding_argument_guards():
    ext = _ext()
    i64 = torch.arange(8, dtype=torch.int64, device="cuda")
    u8 = torch.zeros(16, dtype=torch.uint8, device="cuda")
    e = torch.empty(0, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ext.zorder_key([i64, i64], 33)
    with pytest.raises(RuntimeError):
        ext.zorder_key([i64], 65)
    with pytest.raises(RuntimeError):
        ext.zorder_key([i64], -1)
    with pytest.raises(RuntimeError):
        ext.rle_decode(u8, e, e, e, e, e, 33, 0)
    with pytest.raises(RuntimeError):
        ext.rle_decode(u8, e, e, e, e, e, -1, 0)
    with pytest.raises(RuntimeError):
        ext.murmur3_bucket([i64], 0)
    with pytest.raises(RuntimeError):
        ext.murmur3_bucket([i64], -5)
    words = torch.zeros(1, dtype=torch.int64, device="cuda")
    for m_bits, k in ((0, 3), (-64, 3), (64, -1)):
        with pytest.raises(RuntimeError):
            ext.bloom_build(i64, m_bits, k)
        with pytest.raises(RuntimeError):
            ext.bloom_probe(i64, words, m_bits, k)
        with pytest.raises(RuntimeError):
            ext.bloom_probe_many(i64, words.reshape(1, 1), m_bits, k)
    # the accepted edges still run
    assert ext.zorder_key([i64], 64).numel() == 8
    assert ext.rle_decode(u8, e, e, e, e, e, 0, 0).numel() == 0
    assert ext.bloom_build(i64, 64, 0).cpu().tolist() == [0]
