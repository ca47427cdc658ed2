"""Plain numpy reference of the count step's row operations, for rows a test engineers itself
(hga_count_add_rows, or device buffers handed to the merges) instead of counting them from reads.

Rows are (keys u64 [n], counts [n][F]).  Every sum is taken in uint64 / Python ints; the one float
expression (the specificity of JellyfishOccurrenceReader.cpp:103) is evaluated in Python floats,
i.e. IEEE doubles with one rounding per operation.  tests/test_rows_ref.py pins these functions to
the oracle on small random cases."""
import numpy as np

U32_MAX = (1 << 32) - 1


def _rows(keys, counts):
    keys = np.ascontiguousarray(keys, np.uint64)
    counts = np.asarray(counts)
    if counts.ndim == 1:   # one file
        counts = counts.reshape(len(keys), 1)
    return keys, counts.astype(np.uint64)


def from_dumps(dumps):
    """Per-file dumps [(keys, counts[n])] of F files -> F sources (keys, counts[n][F]) for merge()."""
    F = len(dumps)
    out = []
    for f, (k, c) in enumerate(dumps):
        cc = np.zeros((len(k), F), np.uint64)
        cc[:, f] = c
        out.append((np.asarray(k, np.uint64), cc))
    return out


def merge(sources, min_per_file, saturate=True):
    """Sum per key and file over all sources (saturate: each sum capped at 2^32 - 1, the rule of
    exchange.hip's merge_bucket and kx_run_sum), per-file drop c < min -> 0, rows whose counts are all
    zero dropped.  Returns (keys ascending, counts[rows][F]), u32 when saturating, else u64."""
    parts = [_rows(k, c) for k, c in sources]
    F = parts[0][1].shape[1]
    keys = np.concatenate([p[0] for p in parts])
    cnts = np.concatenate([p[1].reshape(-1, F) for p in parts])
    u, inv = np.unique(keys, return_inverse=True)
    tot = np.zeros((len(u), F), np.uint64)
    np.add.at(tot, inv.reshape(-1), cnts)
    if saturate:
        tot = np.minimum(tot, np.uint64(U32_MAX))
    tot[tot < np.uint64(min_per_file)] = 0
    keep = tot.any(axis=1)
    return u[keep], tot[keep].astype(np.uint32 if saturate else np.uint64)


def spec_index(max_c, sum_c, thresholds):
    """The number of thresholds <= (max / sum) * 100 (std::set<double>::upper_bound)."""
    x = (float(max_c) / float(sum_c)) * 100
    return sum(1 for t in thresholds if t <= x)


def spec_hist(counts, thresholds):
    """(threshold index, total, rows) triples ordered by index, then total (int64 [n][3]).  A row at or
    above the last threshold raises ValueError, as the reference's map lookup would fail."""
    counts = np.asarray(counts).astype(np.uint64)
    if len(counts) == 0:
        return np.zeros((0, 3), np.int64)
    counts = counts.reshape(len(counts), -1)
    thr = sorted(set(float(t) for t in thresholds))
    pairs, n = np.unique(np.stack([counts.max(axis=1), counts.sum(axis=1)], axis=1), axis=0, return_counts=True)
    bins = {}
    for (mx, tot), rows in zip(pairs.tolist(), n.tolist()):
        ti = spec_index(mx, tot, thr)
        if ti == len(thr):
            raise ValueError("a row's specificity is above the last threshold")
        bins[(ti, tot)] = bins.get((ti, tot), 0) + rows
    return np.array([[ti, tot, bins[(ti, tot)]] for ti, tot in sorted(bins)], np.int64).reshape(-1, 3)


def select(keys, counts, lower, upper):
    """(keys with lower <= total <= upper ascending, flag per key: present in exactly one file, the
    number of flags set)."""
    keys, counts = _rows(keys, counts)
    order = np.argsort(keys, kind="stable")
    keys, counts = keys[order], counts[order]
    tot = [int(t) for t in counts.sum(axis=1).tolist()]
    keep = np.array([lower <= t <= upper for t in tot], bool).reshape(-1)
    flags = ((counts > 0).sum(axis=1) == 1)[keep].astype(np.uint8)
    return keys[keep], flags, int(flags.sum())


def dump(keys, counts, f):
    """File f's dump: the rows with a nonzero count there, ascending."""
    keys, counts = _rows(keys, counts)
    order = np.argsort(keys, kind="stable")
    keys, c = keys[order], counts[order, f]
    return keys[c > 0], c[c > 0].astype(np.uint32)


def pack_bits(k, F):
    """Bits per file count of the packed row format (include/hga.h, hga_count_pack_bits):
    (64 - 2k) / F, at most 32; 0 (not packable) when below 4 or with more than 8 files."""
    cb = (64 - 2 * k) // F
    return min(cb, 32) if F <= 8 and cb >= 4 else 0


def pieces_per_row(counts, k, F):
    """Pieces each row travels as: ceil(largest count / (2^bits - 1)), at least one."""
    cmax = (1 << pack_bits(k, F)) - 1
    big = np.asarray(counts).astype(np.uint64).reshape(len(counts), F).max(axis=1)
    return np.maximum((big + np.uint64(cmax - 1)) // np.uint64(cmax), np.uint64(1)).astype(np.int64)


def pieces(keys, counts, k, F):
    """The rows in the packed format: key in the low 2k bits, file f's count in the `bits` bits from
    2k + f * bits.  A row whose largest count exceeds 2^bits - 1 becomes several pieces with the same
    key, filled greedily: every piece takes min(what is left, 2^bits - 1) of each file."""
    bits = pack_bits(k, F)
    assert bits > 0, "rows of this k / file count do not pack"
    keys, counts = _rows(keys, counts)
    cmax = np.uint64((1 << bits) - 1)
    npc = pieces_per_row(counts, k, F)
    row = np.repeat(np.arange(len(keys)), npc)
    nth = (np.arange(len(row)) - np.repeat(np.cumsum(npc) - npc, npc)).astype(np.uint64)
    taken = nth[:, None] * cmax
    c = counts[row]
    part = np.where(c > taken, np.minimum(c - np.minimum(taken, c), cmax), np.uint64(0))
    out = keys[row].copy()
    for f in range(F):
        out |= part[:, f] << np.uint64(2 * k + f * bits)
    return out


def unpack(pcs, k, F):
    """Packed pieces -> (keys, counts[n][F] u64), one row per piece."""
    bits = pack_bits(k, F)
    pcs = np.ascontiguousarray(pcs, np.uint64)
    cmax = np.uint64((1 << bits) - 1)
    keys = pcs & np.uint64((1 << (2 * k)) - 1)
    counts = np.stack([(pcs >> np.uint64(2 * k + f * bits)) & cmax for f in range(F)], axis=1)
    return keys, counts
