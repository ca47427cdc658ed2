"""The owner exchange (csrc/exchange.hip, comm.hip) beyond two packable files.

(1) The caller-driven merges and partitions fed directly: hga_count_merge (wide rows) and
    hga_count_merge_packed with 1 to 64 files, every FMAX instance of kx_mb_merge, pieces of 4 to 32 bits,
    rows split into many pieces and sums that pass 2^32 - 1 (they saturate there); hga_count_partition /
    hga_count_partition_packed on engineered rows, three owners, one of them empty.  The reference is
    tests/rows_ref.py.
(2) hga_count_exchange on a one-rank RCCL communicator with 2 to 9 files: shapes that pack (the FMAX = 4
    and 8 instances of kx_xb_merge, the sender's own binning with split rows) and shapes that do not (the
    wide branch of exchange_protocol.hpp count_exchange: the product's default of two files at k >= 29);
    launch counts prove which branch ran.  The reference is the oracle over all reads.
The several-process cases of the same shapes are in test_dist_gpu.py."""
import numpy as np
import pytest
import torch

import hga
import oracle
import rows_ref
from test_count_rows_gpu import (T8, check_all, check_hist, check_rows, check_select, load_rows, random_keys,
                                 split3)
from test_dist import make_streams

pytestmark = pytest.mark.gpu
THR = oracle.THRESHOLDS
U32_MAX = rows_ref.U32_MAX


# ---- device buffers --------------------------------------------------------------------------------
def dev_from(a):
    """A numpy array of u64 / u32 on the device (torch tensor; data_ptr() is what the C ABI takes)."""
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype.itemsize == 8 else np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    return t


def dev_empty(n, dtype):
    return torch.zeros(max(n, 1), dtype=torch.int64 if np.dtype(dtype).itemsize == 8 else torch.int32, device="cuda:0")


def host_of(t, n, dtype):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)[:n].copy()


def hga_status(code):
    return pytest.raises(hga.HgaError, match=f"hga status {code}")


# ---- 1a. hga_count_merge ---------------------------------------------------------------------------
def wide_sources(rng, k, F, saturating):
    """4 sources of 5000 rows over 8000 keys (at most one row per key and source), counts 0-6; with
    `saturating`, three more keys whose sums over the sources pass 2^32 - 1 in the first and last file."""
    keys = random_keys(rng, k, 8003)
    universe, sat = keys[:8000], keys[8000:]
    out = []
    for s in range(4):
        ks = universe[rng.permutation(8000)[:5000]]
        cs = rng.integers(0, 7, (5000, F)).astype(np.uint32)
        cs[rng.random((5000, F)) < 0.3] = 0
        empty = ~cs.any(axis=1)
        cs[empty, rng.integers(0, F, int(empty.sum()))] = 1
        if saturating:
            sc = np.ones((3, F), np.uint32)
            sc[:, 0] = sc[:, F - 1] = (1 << 31) if s < 3 else 5
            ks, cs = np.concatenate([ks, sat]), np.concatenate([cs, sc])
        order = rng.permutation(len(ks))
        out.append((ks[order], cs[order]))
    return out


@pytest.mark.parametrize("min_c", [1, 3])
@pytest.mark.parametrize("k,F", [(19, 1), (19, 3), (32, 2), (11, 9), (19, 64)])
def test_merge_wide(gpu_ctx, k, F, min_c):
    """kx_merge_flags / kx_merge_emit on 20 000 rows from 4 sources: sums, the per-file drop, saturation
    at 2^32 - 1 (kx_run_sum), then every row query on the merged rows."""
    for saturating in (True, False):
        src = wide_sources(np.random.default_rng(100 * k + F), k, F, saturating)
        rk, rc = rows_ref.merge(src, min_c)
        keys = np.concatenate([s[0] for s in src])
        counts = np.concatenate([s[1] for s in src])
        assert 20_000 <= len(keys) <= 20_012 and len(rk) < len(keys)
        if saturating:   # 3 x 2^31 (+ 5) in the reference's exact sums
            exact = rows_ref.merge(src, min_c, saturate=False)[1]
            assert int(exact.max()) == 3 * (1 << 31) + 5 and int((rc == U32_MAX).sum()) == (3 if F == 1 else 6)
        kt, ct = dev_from(keys), dev_from(counts.reshape(-1))
        gpu_ctx.count_begin(k, F)
        gpu_ctx.count_merge(kt.data_ptr(), ct.data_ptr(), len(keys), min_c)
        if saturating:   # totals of 2^31 and more: rows and dumps only
            check_rows(gpu_ctx, rk, rc)
        else:
            check_all(gpu_ctx, rk, rc, bounds=((1, 2 ** 31 - 1), (5, 12)))


# ---- 1b. hga_count_merge_packed --------------------------------------------------------------------
VALUES = np.array([0, 1, 15, 16, 30, 31, 1000], np.uint32)   # at 4 bits per count every count >= 16 splits
WEIGHTS = np.array([0.36, 0.3, 0.1, 0.1, 0.06, 0.06, 0.02])
PIECES = 50_000


def packed_sources(rng, k, F, saturating=False):
    """Sources of rows with counts from VALUES (at most one row per key and source), cut so that all
    sources together travel as at most PIECES pieces; with `saturating` (a piece holds a whole u32),
    three keys whose sums over three sources are 3 x 2^31."""
    n_keys = min(1 << (2 * k), 20_000)
    keys = random_keys(rng, k, n_keys)
    universe, sat = keys[:n_keys - 3], keys[n_keys - 3:]
    n_src = 3 if n_keys == 20_000 else 40   # k = 5 has 1024 keys only
    out = []
    for s in range(n_src):
        ks = rng.permutation(universe)[:PIECES // n_src]
        cs = VALUES[rng.choice(len(VALUES), (len(ks), F), p=WEIGHTS)]
        empty = ~cs.any(axis=1)
        cs[empty, rng.integers(0, F, int(empty.sum()))] = 1
        fit = int(np.searchsorted(np.cumsum(rows_ref.pieces_per_row(cs, k, F)), PIECES // n_src, side="right"))
        ks, cs = ks[:fit], cs[:fit]
        if saturating and s < 3:
            ks, cs = np.concatenate([ks, sat]), np.concatenate([cs, np.full((3, F), 1 << 31, np.uint32)])
        out.append((ks, cs))
    return out


@pytest.mark.parametrize("k,F,min_c", [(16, 1, 2), (5, 1, 1), (19, 3, 2), (19, 4, 1), (19, 5, 2), (13, 8, 2), (16, 8, 3),
                                       (19, 1, 2)])
def test_merge_packed(gpu_ctx, k, F, min_c):
    """kx_mb_merge<2048, 2>, <1024, 4> and <1024, 8> on about 50 000 pieces of 32, 26, 8, 6, 5 and 4 bits per
    count: rows split into up to 67 pieces are summed again, sums past 2^32 - 1 saturate."""
    rng = np.random.default_rng(100 * k + F)
    bits = rows_ref.pack_bits(k, F)
    saturating = bits == 32
    src = packed_sources(rng, k, F, saturating)
    pcs = [rows_ref.pieces(ks, cs, k, F) for ks, cs in src]
    n_rows = sum(len(s[0]) for s in src)
    if (k, F) == (19, 1):   # one key in 70 pieces of 2^26 - 1: the sum wraps a u32 at a piece width below 32
        assert bits == 26
        hot = np.full(70, random_keys(rng, k, 1)[0], np.uint64)
        src.append((hot, np.full((70, 1), (1 << 26) - 1, np.uint64)))
        pcs.append(hot | np.uint64(((1 << 26) - 1) << 38))
        saturating = True
    rk, rc = rows_ref.merge(src, min_c)
    pieces = rng.permutation(np.concatenate(pcs))
    assert 30_000 < len(pieces) <= PIECES + 100
    if bits < 10:   # 1000 does not fit a piece (at 4 bits neither do 16-31): more pieces than rows
        assert len(pieces) > (2 if bits == 4 else 1.05) * n_rows
    if saturating:
        exact = rows_ref.merge(src, min_c, saturate=False)[1]
        assert int(exact.max()) > U32_MAX and int((rc == U32_MAX).sum()) == (1 if k == 19 else 3)
    gpu_ctx.count_begin(k, F)
    assert gpu_ctx.count_pack_bits() == bits > 0
    pt = dev_from(pieces)
    gpu_ctx.count_merge_packed(pt.data_ptr(), len(pieces), min_c)
    if saturating:
        check_rows(gpu_ctx, rk, rc)
    else:
        check_all(gpu_ctx, rk, rc, bounds=((1, 2 ** 31 - 1), (16, 1015)))


@pytest.mark.parametrize("k,F", [(19, 7), (31, 1), (11, 9)])
def test_packed_calls_refuse_unpackable_shapes(gpu_ctx, k, F):
    """Fewer than 4 bits per count, or more than 8 files: hga_count_pack_bits is 0 and the packed calls
    return HGA_ERR_INVALID (the wide form is the one to use)."""
    rng = np.random.default_rng(k + F)
    keys = random_keys(rng, k, 50)
    counts = rng.integers(1, 9, (50, F)).astype(np.uint32)
    load_rows(gpu_ctx, k, keys, counts)
    assert gpu_ctx.count_pack_bits() == rows_ref.pack_bits(k, F) == 0
    buf = dev_empty(64, np.uint64)
    with hga_status(1):
        gpu_ctx.count_partition_packed(np.zeros(0, np.uint64), buf.data_ptr(), 64)
    with hga_status(1):
        gpu_ctx.count_merge_packed(buf.data_ptr(), 8, 1)
    check_rows(gpu_ctx, *rows_ref.merge([(keys, counts)], 1))   # the rows are still there


# ---- 1c. partitions --------------------------------------------------------------------------------
def partition_rows(k, F, n=6000):
    rng = np.random.default_rng(7 * k + F)
    keys = random_keys(rng, k, n)
    counts = VALUES[rng.choice(len(VALUES), (n, F), p=WEIGHTS)]
    empty = ~counts.any(axis=1)
    counts[empty, rng.integers(0, F, int(empty.sum()))] = 1
    return (keys, counts) + rows_ref.merge([(keys, counts)], 1)


@pytest.mark.parametrize("k,F", [(19, 3), (13, 8), (11, 9)])
def test_partition_wide(gpu_ctx, k, F):
    """kx_owner_hist / kx_scatter: 6000 rows (two tiles) to three owners of which the middle one's code
    range is empty; every slice holds exactly its owner's rows."""
    keys, counts, rk, rc = partition_rows(k, F)
    spl = np.array([rk[len(rk) // 3]] * 2, np.uint64)
    owner = np.searchsorted(spl, rk, side="right")
    want = np.bincount(owner, minlength=3)
    assert want[1] == 0 and want[0] > 0 and want[2] > 0
    load_rows(gpu_ctx, k, keys, counts)
    kb, cb = dev_empty(len(rk), np.uint64), dev_empty(len(rk) * F, np.uint32)
    per = gpu_ctx.count_partition(spl, kb.data_ptr(), cb.data_ptr()).astype(np.int64)
    assert per.tolist() == want.tolist()
    ok, oc = host_of(kb, len(rk), np.uint64), host_of(cb, len(rk) * F, np.uint32).reshape(-1, F)
    off = np.concatenate([[0], np.cumsum(per)])
    for o in range(3):
        sl = slice(off[o], off[o + 1])
        order = np.argsort(ok[sl])
        assert np.array_equal(ok[sl][order], rk[owner == o]) and np.array_equal(oc[sl][order], rc[owner == o])


@pytest.mark.parametrize("k,F", [(19, 3), (13, 8)])
def test_partition_packed(gpu_ctx, k, F):
    """kx_piece_hist / kx_pack_scatter with rows that split (the left[] loop over 3 and 8 files): the
    pieces of every owner are exactly the reference's, after a first call with too little room."""
    keys, counts, rk, rc = partition_rows(k, F)
    spl = np.array([0, rk[len(rk) // 2]], np.uint64)   # the first owner's range [.., 0) is empty
    owner = np.searchsorted(spl, rk, side="right")
    npc = rows_ref.pieces_per_row(rc, k, F)
    want = np.bincount(owner, weights=npc, minlength=3).astype(np.int64)
    assert want[0] == 0 and want[1] > 0 and want[2] > 0 and int(want.sum()) > 1.02 * len(rk)
    load_rows(gpu_ctx, k, keys, counts)
    assert gpu_ctx.count_pack_bits() == rows_ref.pack_bits(k, F)
    cap = len(rk) // 4   # deliberately small: nothing is written, the total comes back
    small = dev_from(np.full(cap, 0x5A5A5A5A5A5A5A5A, np.uint64))
    per, tot = gpu_ctx.count_partition_packed(spl, small.data_ptr(), cap)
    assert tot == int(want.sum()) > cap and per.astype(np.int64).tolist() == want.tolist()
    assert (host_of(small, cap, np.uint64) == 0x5A5A5A5A5A5A5A5A).all()
    buf = dev_empty(tot, np.uint64)
    per, tot = gpu_ctx.count_partition_packed(spl, buf.data_ptr(), tot)
    assert tot == int(want.sum()) and per.astype(np.int64).tolist() == want.tolist()
    got = host_of(buf, tot, np.uint64)
    off = np.concatenate([[0], np.cumsum(want)])
    for o in range(3):
        ref = rows_ref.pieces(rk[owner == o], rc[owner == o], k, F)
        assert np.array_equal(np.sort(got[off[o]:off[o + 1]]), np.sort(ref))
    pk, pc = rows_ref.unpack(got, k, F)
    mk, mc = rows_ref.merge([(pk, pc)], 1)
    assert np.array_equal(mk, rk) and np.array_equal(mc, rc)


# ---- 2. hga_count_exchange on a one-rank RCCL communicator -----------------------------------------
def launches(ctx, *names):
    return [ctx.profile_get(n)[1] for n in names]


@pytest.mark.parametrize("k,F,heavy", [(19, 3, False), (19, 5, True), (13, 8, False),        # pack: 8, 5, 4 bits
                                       (31, 2, False), (32, 2, False), (27, 3, False), (11, 9, False)])
def test_rccl_one_rank_exchange_file_counts(k, F, heavy):
    streams = make_streams(heavy=heavy, n_files=F)
    assert len(streams) == F
    ref = oracle.count_pipeline(streams, k, 3, 40)
    packs = rows_ref.pack_bits(k, F) > 0
    if heavy:   # counts past the 5 bits of a piece: rows travel as several pieces
        assert rows_ref.pack_bits(k, F) == 5 and int(ref["counts"].max()) > 31
    with hga.Ctx(0) as ctx:
        ctx.comm_init(hga.comm_unique_id(), 0, 1)
        ctx.count_begin(k, F)
        for f, s in enumerate(streams):
            ctx.count_add(f, s)
        ctx.count_run(1)
        assert (ctx.count_pack_bits() > 0) == packs
        ctx.profile(True)
        try:
            ctx.profile_reset()
            ctx.count_exchange(2)
            wide, packed, binned = launches(ctx, "kx_merge", "kx_xb_merge", "kx_xb_scatter")
        finally:
            ctx.profile(False)
        if packs:   # hash-bucket owners; with more than two files the sender bins its rows itself
            assert packed > 0 and wide == 0 and binned > 0
        else:       # code-range owners: partition, two all-to-alls, merge
            assert wide > 0 and packed == 0 and binned == 0
        assert ctx.count_stats().distinct_rows == len(ref["keys"])
        assert ctx.count_stats().instances == sum(oracle.count_instances(x, k) for x in streams)
        assert np.array_equal(ctx.spec_hist(THR), ref["hist"])
        keys, flags, nd = ctx.select(3, 40)
        assert np.array_equal(keys, ref["selected"]) and nd == ref["n_discr"] == int(flags.sum())
        rk, rc = ctx.rows()
        assert np.array_equal(rk, ref["keys"]) and np.array_equal(rc, ref["counts"])
        for f in (0, F - 1):
            d = ctx.dump(f)
            assert np.array_equal(d[0], ref["dumps"][f][0]) and np.array_equal(d[1], ref["dumps"][f][1])
        ctx.comm_destroy()


def test_rccl_one_rank_exchange_of_rows_large_histogram():
    """Rows from hga_count_add_rows on a ctx with a communicator (they are binned by the sender, as cached
    dumps are), 3000 distinct totals: more (threshold, total) bins than one gather slot holds, so the
    global histogram takes the variable-size gather."""
    k, F, min_c = 19, 3, 2
    rng = np.random.default_rng(8)
    counts = np.array([split3(rng, t) for t in range(1, 3001)], np.uint32)
    keys = random_keys(rng, k, len(counts))
    rk, rc = rows_ref.merge([(keys, counts)], min_c)
    ref_hist = rows_ref.spec_hist(rc, T8)
    assert len(ref_hist) > 1024 and len(rk) < len(keys)
    assert int(rc.max()) > 255   # 8 bits per count: split rows
    with hga.Ctx(0) as ctx:
        ctx.comm_init(hga.comm_unique_id(), 0, 1)
        load_rows(ctx, k, keys, counts)
        ctx.profile(True)
        try:
            ctx.profile_reset()
            ctx.count_exchange(min_c)
            wide, packed = launches(ctx, "kx_merge", "kx_xb_merge")
        finally:
            ctx.profile(False)
        assert packed > 0 and wide == 0
        assert ctx.count_stats().distinct_rows == len(rk)
        check_hist(ctx, rc, T8)
        check_select(ctx, rk, rc, 1000, 1100)
        check_select(ctx, rk, rc, 1, 2 ** 31 - 1)
        got_k, got_c = ctx.rows()
        assert np.array_equal(got_k, rk) and np.array_equal(got_c, rc)
        for f in range(F):
            d = ctx.dump(f)
            w = rows_ref.dump(rk, rc, f)
            assert np.array_equal(d[0], w[0]) and np.array_equal(d[1], w[1])
        ctx.comm_destroy()
