"""cut_records (host/fastio.cpp): the piece starts bin/jf_occurrences --device-parse hands to
hga_count_add_file.  No GPU: the pieces go through the host reader instead of the device parser."""
import random

import pytest

import ingest_cases as ic

PIECES = [1, 64, 4096, 1 << 40]


@pytest.fixture(scope="module")
def hga(hga_mod):
    hga_mod.set_host_threads(1)   # the sequential reader is the oracle
    yield hga_mod
    hga_mod.set_host_threads(0)


def files(seed):
    return ic.fuzz_files(seed, 30, 20000)


def line_starts(data):
    return {0} | {i + 1 for i, b in enumerate(data) if b == 10 and i + 1 < len(data)}


def is_record_start(data, at, starts):
    """The definition in seqio.h, on the file's own lines."""
    first = data.lstrip(b"\n")[:1]
    if at not in starts:
        return False
    if first == b">":
        return data[at:at + 1] == b">"
    if data[at:at + 1] != b"@":
        return False
    rest = data[at:].split(b"\n", 3)
    return len(rest) > 2 and rest[2][:1] == b"+"


@pytest.mark.parametrize("piece", PIECES)
def test_cut_starts_are_record_starts(hga, piece):
    for fam, data in files(11):
        cuts = [int(c) for c in hga.cut_records(data, piece)]
        assert cuts[0] == 0 and all(a < b for a, b in zip(cuts, cuts[1:])) and cuts[-1] < max(1, len(data)), (fam, cuts)
        starts = line_starts(data)
        first = data.lstrip(b"\n")[:1]
        if first not in (b">", b"@"):
            assert cuts == [0]
            continue
        for c in cuts[1:]:
            assert is_record_start(data, c, starts), (fam, piece, c)
            # the first one at or after the next multiple of piece above the previous start
            prev = max(x for x in cuts if x < c)
            m = (prev // piece + 1) * piece
            assert m <= c and not any(is_record_start(data, x, starts) for x in sorted(starts) if m <= x < c), (fam, piece, c)
        if piece >= len(data):
            assert cuts == [0]


@pytest.mark.parametrize("piece", PIECES)
def test_cut_pieces_hold_the_same_reads(hga, piece):
    """Accepted files: the reads of the pieces, in order, are the file's reads (an empty piece adds no
    separator, so empty reads are dropped on both sides; one piece is the file, byte for byte)."""
    for fam, data in files(12):
        if fam == "refused":
            continue
        whole = ic.oracle_stream(hga, data)
        cuts = [int(c) for c in hga.cut_records(data, piece)] + [len(data)]
        streams = [ic.oracle_stream(hga, data[a:b]) for a, b in zip(cuts, cuts[1:])]
        if len(streams) == 1:
            assert streams[0] == whole
        reads = [r for s in streams for r in s.split(b"\n") if r]
        assert reads == [r for r in whole.split(b"\n") if r], (fam, piece)
        # every piece of an accepted file is accepted by the device's rule (leading empty lines: empty)
        for a, b in zip(cuts, cuts[1:]):
            assert ic.expected_layout(data[a:b])[0] in (ic.FAMILIES[fam][1], ic.EMPTY), (fam, piece, a, b)


def test_cut_edges(hga):
    assert list(hga.cut_records(b"", 16)) == [0]
    assert list(hga.cut_records(b"\n\n\n\n", 1)) == [0]
    assert list(hga.cut_records(b"ACGT\n>h\nAC\n", 1)) == [0]
    assert list(hga.cut_records(b">a\nAC\n>b\nGT\n>c", 1)) == [0, 6, 12]
    assert list(hga.cut_records(b">a\nAC\n>b\nGT\n>c", 7)) == [0, 12]
    # a quality line starting with '@' is not a start: two lines below it lies a sequence line
    fq = b"@r0\nACGT\n+\n@III\n@r1\nAC\n+\n@I\n"
    assert list(hga.cut_records(fq, 1)) == [0, 16]
    assert list(hga.cut_records(fq, 12)) == [0, 16]
    with pytest.raises(hga.HgaError):
        hga.cut_records(fq, 0)
    rng = random.Random(3)
    big = ic.gen_fastq(rng, 3000)
    assert list(hga.cut_records(big, len(big))) == [0]


def test_cut_records_under_sanitizers(tmp_path):
    """tests/native/ingest_cut_check.cpp with the host reader's sources under AddressSanitizer + UBSan, as a
    program of its own: inputs in heap blocks of exactly their size."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "hybrid-genome-assembler_amd", "host")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "ingest_cut_check")
    b = subprocess.run([cxx, "-O0", "-g", "-std=c++20", "-pthread", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", host,
                        "-I", os.path.join(root, "include"), os.path.join(root, "tests", "native", "ingest_cut_check.cpp"),
                        os.path.join(host, "fastio.cpp"), os.path.join(host, "seqio.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert r.stdout.strip().endswith(" 0 failures")
