"""hga_count_add_file on the MI355X: FASTA / FASTQ parsed on the device.  The oracle for the bytes is the
sequential host reader (hga.jf_stream with one reader thread), for the layout the acceptance rule of
include/hga.h restated in ingest_cases.expected_layout.  Every case asserts the info, the resident stream
byte for byte, and for a refused file that the ctx is as before the call.  Sizes are in units of the
parser's tile T (hga_ingest_tile): the smallest that reach each boundary."""
import functools
import random

import numpy as np
import pytest

import ingest_cases as ic
import oracle
from test_count_passes_gpu import assert_equal_runs, assert_same, fetch

pytestmark = pytest.mark.gpu

HGA_ERR_INVALID, HGA_ERR_STATE = 1, 4


@pytest.fixture(scope="module")
def hga(hga_mod):
    hga_mod.set_host_threads(1)   # the sequential reader is the oracle
    yield hga_mod
    hga_mod.set_host_threads(0)


@pytest.fixture
def ctx(gpu_ctx, hga):
    return gpu_ctx


def expect(hga, data):
    lay, rec, lines = ic.expected_layout(data)
    want = ic.oracle_stream(hga, data) if lay in (ic.FASTA, ic.FASTQ) else b""
    return {"layout": lay, "records": rec, "lines": lines, "seq_bytes": len(want)}, want


def check(hga, ctx, data, layout=None, prefix=b"ACGTN"):
    """One call on an empty file and one behind `prefix`; returns the expected layout."""
    info, want = expect(hga, data)
    if layout is not None:
        assert info["layout"] == layout, "the case is not of the layout it was written for"
    ctx.count_begin(19, 1)
    assert ctx.count_add_file(0, data) == info
    assert ctx.count_seq(0) == want
    ctx.count_begin(19, 1)
    ctx.count_add(0, prefix)
    assert ctx.count_add_file(0, data) == info
    assert ctx.count_seq(0) == prefix + (b"\n" + want if want else b"")
    return info["layout"]


def fa_exact(size, newline=True):
    """A FASTA file of exactly `size` bytes: one header, one sequence line."""
    body = size - 3 - (1 if newline else 0)
    return b">h\n" + (b"ACGTacgtN" * (body // 9 + 1))[:body] + (b"\n" if newline else b"")


def fq_exact(size):
    """A one-record FASTQ file of exactly `size` bytes."""
    plus = b"+" if size % 2 else b"+x"
    n = (size - 6 - len(plus)) // 2
    seq = (b"ACGTacgtN" * (n // 9 + 1))[:n]
    data = b"@h\n" + seq + b"\n" + plus + b"\n" + b"I" * n + b"\n"
    assert len(data) == size
    return data


def tile_cases(T):
    fa_pad = lambda n: b">h\n" + b"A" * (n - 4) + b"\n"   # n bytes, the last one a newline
    c = {}
    for name, size in (("T-1", T - 1), ("T", T), ("T+1", T + 1), ("2T+1", 2 * T + 1)):
        c[f"fasta_{name}"] = (fa_exact(size), ic.FASTA)
        c[f"fasta_{name}_no_newline"] = (fa_exact(size, False), ic.FASTA)
        c[f"fastq_{name}"] = (fq_exact(size), ic.FASTQ)
    c["newline_last_of_tile"] = (fa_pad(T) + b"CC\n", ic.FASTA)
    c["newline_first_of_tile"] = (fa_pad(T + 1) + b"CC\n", ic.FASTA)
    c["newline_last_and_first"] = (fa_pad(T) + b"\nCC\n", ic.FASTA)
    c["header_first_of_tile"] = (fa_pad(T) + b">h2\nCC\n", ic.FASTA)
    c["sequence_gt_first_of_tile"] = (b">h\n" + b"A" * (T - 3) + b">CC\nGG\n", ic.FASTA)   # '>' inside a line
    c["at_first_of_tile"] = (fq_exact(T) + fq_exact(41), ic.FASTQ)
    c["at_first_of_tile_fasta_line"] = (fa_pad(T) + b"@CC\n+GG\n", ic.FASTA)
    long_line = (b"ACGTacgtNn" * (3 * T // 10 + 2))[:3 * T + 7]
    c["fasta_line_over_3_tiles"] = (b">h\nAC\n" + long_line + b"\nGG\n>h2\n" + long_line, ic.FASTA)
    c["fastq_line_over_3_tiles"] = (b"@h\n" + long_line + b"\n+\n" + b"I" * len(long_line) + b"\n@h2\nAC\n+\nII\n", ic.FASTQ)
    c["fasta_header_over_edge"] = (b">" + b"h" * (T + 10) + b"\nACGT\n", ic.FASTA)
    c["fasta_second_header_over_edge"] = (fa_pad(T - 5) + b">hhhhhhhhhh\nGG\n", ic.FASTA)
    c["fasta_header_over_3_tiles"] = (b">a\nAC\n>" + b"h" * (3 * T) + b"\nGG\n", ic.FASTA)
    c["fastq_header_over_edge"] = (b"@" + b"h" * (T + 3) + b"\nAC\n+\nII\n" + fq_exact(33), ic.FASTQ)
    c["fastq_quality_over_edge"] = (fq_exact(2 * T - 9) + fq_exact(35), ic.FASTQ)
    c["only_newlines_4T"] = (b"\n" * (4 * T), ic.EMPTY)
    c["fasta_one_byte_lines_4T"] = (b">\n" + b"A\n" * (4 * T - 1), ic.FASTA)
    c["fasta_one_byte_headers_4T"] = (b">\n" * (4 * T), ic.FASTA)
    c["fastq_one_byte_lines_4T"] = (b"@\nA\n+\nI\n" * T, ic.FASTQ)
    return c


SMALL = {
    # ends
    "empty": (b"", ic.EMPTY),
    "one_newline": (b"\n", ic.EMPTY),
    "fasta_no_trailing_newline": (b">h\nACGT\n>h2\nGG", ic.FASTA),
    "fasta_trailing_two_newlines": (b">h\nACGT\n\n", ic.FASTA),
    "fastq_no_trailing_newline": (b"@h\nACGT\n+\nIIII", ic.FASTQ),
    "fastq_trailing_two_newlines": (b"@h\nACGT\n+\nIIII\n\n", ic.REFUSED),
    "fasta_leading_empty_lines": (b"\n\n\n>h\nACGT\n>h2\nGG\n", ic.FASTA),
    "fastq_leading_empty_line": (b"\n@h\nACGT\n+\nIIII\n", ic.REFUSED),
    "header_without_newline": (b">", ic.FASTA),
    "at_without_newline": (b"@", ic.REFUSED),
    # FASTA
    "fasta_multi_line": (b">h\nACGT\nGGCC\nTT\n>h2\nAAAA\nCC\n", ic.FASTA),
    "fasta_at_and_plus_lines": (b">h\n@CGT\n+GCC\n>h2\n+\n@\n", ic.FASTA),
    "fasta_empty_lines_inside": (b">h\nAC\n\n\nGT\n\n>h2\n\nGG\n", ic.FASTA),
    "fasta_headers_only": (b">a\n>b\n>c\n>d\n", ic.FASTA),
    "fasta_one_header": (b">a\n", ic.FASTA),
    "fasta_crlf": (b">h\r\nACGT\r\nGG\r\n>h2\r\nCC\r\n", ic.FASTA),
    "fasta_lowercase_and_n": (b">h\nacgtnNACGTnn\n>h2\nNNNN\n", ic.FASTA),
    "fasta_gt_inside_lines": (b">h>x\nAC>GT\n", ic.FASTA),
    # FASTQ accepted
    "fastq_quality_at_plus": (b"@h\nACGT\n+\n@III\n@h2\nGGCC\n+h2\n+III\n", ic.FASTQ),
    "fastq_empty_sequences": (b"@h\n\n+\n\n@h2\nAC\n+\nII\n@h3\n\n+\n\n", ic.FASTQ),
    "fastq_only_empty_sequence": (b"@h\n\n+\n\n", ic.FASTQ),
    "fastq_crlf": (b"@h\r\nACGT\r\n+\r\nIIII\r\n@h2\r\nGG\r\n+\r\nII\r\n", ic.FASTQ),
    "fastq_one_record": (b"@h\nACGTACGTACGTACGTACGTAC\n+\nIIIIIIIIIIIIIIIIIIIIII\n", ic.FASTQ),
    "fastq_sequence_starts_with_at": (b"@h\n@CGT\n+\nIIII\n", ic.FASTQ),
    # first byte
    "first_byte_A": (b"ACGT\n>h\nACGT\n", ic.REFUSED),
    "first_byte_plus": (b"+\n@h\nAC\n+\nII\n", ic.REFUSED),
    "first_byte_A_after_newlines": (b"\n\nACGT\n", ic.REFUSED),
}


@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_files(hga, ctx, name):
    data, layout = SMALL[name]
    check(hga, ctx, data, layout)


def test_tile_edges(hga, ctx):
    T = hga.ingest_tile()
    assert T >= 64
    for name, (data, layout) in tile_cases(T).items():
        try:
            check(hga, ctx, data, layout)
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("defect", ic.DEFECTS)
def test_fastq_refused(hga, ctx, defect, where):
    """The defect once in the first record and once only in the last one of a file of more than 8 tiles:
    the refusal comes from a far workgroup."""
    T = hga.ingest_tile()
    base = ic.plain_fastq(random.Random(5), 8 * T + 100)
    ls = ic.getlines(base)
    data = ic.apply_defect(ls, 0 if where == "first" else len(ls) - 4, defect)
    assert len(data) > 8 * T
    check(hga, ctx, base, ic.FASTQ)
    check(hga, ctx, data, ic.REFUSED)


def test_calls(hga, ctx):
    T = hga.ingest_tile()
    fa = ic.gen_fasta(random.Random(1), 2 * T)
    fq = ic.gen_fastq(random.Random(2), 2 * T)
    bad = ic.apply_defect(ic.getlines(ic.plain_fastq(random.Random(3), 2 * T)), 0, "qlen")
    (ifa, sfa), (ifq, sfq), (ibad, _) = expect(hga, fa), expect(hga, fq), expect(hga, bad)
    assert (ifa["layout"], ifq["layout"], ibad["layout"]) == (ic.FASTA, ic.FASTQ, ic.REFUSED)
    # two add_file calls on one file; a refused call between two accepted ones; an empty one adds nothing
    ctx.count_begin(19, 1)
    assert ctx.count_add_file(0, fa) == ifa
    assert ctx.count_add_file(0, bad) == ibad
    assert ctx.count_seq(0) == sfa
    assert ctx.count_add_file(0, b"\n\n")["layout"] == ic.EMPTY
    assert ctx.count_add_file(0, b">only\n")["seq_bytes"] == 0
    assert ctx.count_seq(0) == sfa
    assert ctx.count_add_file(0, fq) == ifq
    assert ctx.count_seq(0) == sfa + b"\n" + sfq
    # add then add_file, and the reverse
    ctx.count_begin(19, 1)
    ctx.count_add(0, b"ACGTACGT")
    assert ctx.count_add_file(0, fq) == ifq
    ctx.count_add(0, b"GGGG")
    assert ctx.count_seq(0) == b"ACGTACGT\n" + sfq + b"\nGGGG"
    # file 1 of 2 only; hga_count_begin resets
    ctx.count_begin(19, 2)
    assert ctx.count_seq(0) == b"" and ctx.count_seq(1) == b""
    assert ctx.count_add_file(1, fa) == ifa
    assert ctx.count_seq(0) == b"" and ctx.count_seq(1) == sfa
    ctx.count_begin(19, 2)
    assert ctx.count_seq(1) == b""
    # the same ctx state as count_add(jf_stream): the rows of both routes
    ctx.count_begin(5, 2)
    ctx.count_add_file(0, fa)
    ctx.count_add_file(1, fq)
    ctx.count_run(1)
    got = ctx.rows()
    ctx.count_begin(5, 2)
    ctx.count_add(0, sfa)
    ctx.count_add(1, sfq)
    ctx.count_run(1)
    want = ctx.rows()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_on_a_ctx_with_a_communicator(hga):
    fq = ic.gen_fastq(random.Random(4), 3000)
    info, want = expect(hga, fq)
    with hga.Ctx(0) as c:
        c.comm_init_host(0, 1, hga.transport_of(lambda send, recv: None, 1))
        c.count_begin(19, 1)
        assert c.count_add_file(0, fq) == info
        assert c.count_seq(0) == want


def test_error_rules(hga):
    import ctypes as C
    lib = hga.lib()
    info = hga.IngestInfo()
    with hga.Ctx(0) as c:
        with pytest.raises(hga.HgaError) as e:
            c.count_add_file(0, b">h\nAC\n")
        assert str(e.value).startswith(f"hga status {HGA_ERR_STATE}:")
        with pytest.raises(hga.HgaError) as e:
            c.count_seq(0)
        assert str(e.value).startswith(f"hga status {HGA_ERR_STATE}:")
        c.count_begin(19, 2)
        with pytest.raises(hga.HgaError) as e:
            c.count_add_file(2, b">h\nAC\n")
        assert str(e.value).startswith(f"hga status {HGA_ERR_INVALID}:")
        with pytest.raises(hga.HgaError) as e:
            c.count_seq(2)
        assert str(e.value).startswith(f"hga status {HGA_ERR_INVALID}:")
        assert lib.hga_count_add_file(c._h, 0, None, 5, C.byref(info)) == HGA_ERR_INVALID
        assert lib.hga_count_add_file(c._h, 0, b">h\nAC\n", 6, None) == HGA_ERR_INVALID
        assert lib.hga_count_add_file(c._h, 0, None, 0, C.byref(info)) == 0 and info.layout == ic.EMPTY
        # more than 2^32 - 1 bytes in one call: refused before a byte is read
        assert lib.hga_count_add_file(c._h, 0, b">h\nAC\n", 1 << 32, C.byref(info)) == HGA_ERR_INVALID
        assert c.count_seq(0) == b"" and c.count_seq(1) == b""


def test_seeded_fuzz(hga, ctx):
    """200 files of at most 4 tiles from the three families; each family asserts its own layout."""
    T = hga.ingest_tile()
    seen = {}
    for i, (fam, data) in enumerate(ic.fuzz_files(20260101, 200, 4 * T)):
        info, want = expect(hga, data)
        assert info["layout"] == ic.FAMILIES[fam][1], (i, fam)
        prefix = b"" if i % 2 else b"TTTT"
        ctx.count_begin(19, 1)
        if prefix:
            ctx.count_add(0, prefix)
        assert ctx.count_add_file(0, data) == info, (i, fam, len(data))
        assert ctx.count_seq(0) == (prefix + (b"\n" + want if want else b"") if prefix else want), (i, fam, len(data))
        seen[fam] = seen.get(fam, 0) + 1
    assert min(seen.values()) >= 66 and len(seen) == 3


# ---- counts: two files of about 8 MB through add_file against count_add(jf_stream) and the oracle

@functools.lru_cache(maxsize=None)
def count_files():
    """(raw FASTA bytes, raw FASTQ bytes) of about 8 MB each, and their streams by the sequential reader."""
    import hga
    ga = hga.gen_genome(300_000, 1)
    gb = hga.gen_haplotype(ga, 0.03, 0, 2)
    ra, rb = hga.gen_art(ga, 52_000, 150, 3), hga.gen_art(gb, 26_000, 150, 4)
    reads_a = ra.seq.split(b"\n")
    fa = b"".join(b">read_%d\n%s\n%s\n%s\n" % (i, r[:60], r[60:120], r[120:]) for i, r in enumerate(reads_a))
    fq = b"".join(b"@read_%d/1\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(rb.seq.split(b"\n")))
    hga.set_host_threads(1)
    streams = [ic.oracle_stream(hga, fa), ic.oracle_stream(hga, fq)]
    assert streams[0] == ra.seq and streams[1] == rb.seq
    return (fa, fq), streams


@functools.lru_cache(maxsize=None)
def count_oracle(k, min_count):
    _, streams = count_files()
    o = oracle.count_pipeline_mt(streams, k, 3, 40, threads=8, min_count=min_count)
    o["dumps"] = oracle.dumps_of(o["keys"], o["counts"])
    return o


@pytest.fixture
def pctx(gpu_ctx):
    yield gpu_ctx
    gpu_ctx.count_set_passes(0, 0)


@pytest.mark.parametrize("min_count", [1, 2])
@pytest.mark.parametrize("k", [5, 19, 32])
def test_counts_through_add_file(hga, pctx, k, min_count):
    raw, streams = count_files()
    assert all(7_000_000 < len(r) < 10_000_000 for r in raw)
    o = count_oracle(k, min_count)
    pctx.count_begin(k, 2)
    for f, s in enumerate(streams):
        pctx.count_add(f, s)
    pctx.count_run(min_count)
    by_stream = fetch(pctx, 2, 3, 40)
    assert_same(by_stream, o)
    pctx.count_begin(k, 2)
    assert pctx.count_add_file(0, raw[0])["layout"] == ic.FASTA
    assert pctx.count_add_file(1, raw[1])["layout"] == ic.FASTQ
    est = pctx.count_estimate(min_count, 1)
    pctx.count_run(min_count)
    by_file = fetch(pctx, 2, 3, 40)
    assert_same(by_file, o)
    assert_equal_runs(by_file, by_stream)
    assert by_file["pass_stats"].work_bytes == by_stream["pass_stats"].work_bytes == est
    # the same input in four key-range passes
    pctx.count_set_passes(4, 0)
    pctx.count_begin(k, 2)
    pctx.count_add_file(0, raw[0])
    pctx.count_add_file(1, raw[1])
    pctx.count_run(min_count)
    by_passes = fetch(pctx, 2, 3, 40)
    assert_same(by_passes, o)
    assert_equal_runs(by_passes, by_file)
    assert by_passes["pass_stats"].passes == (4 if k >= 12 else by_passes["pass_stats"].passes)
