"""Shared by the device-parser tests (test_ingest_gpu.py, test_ingest_cut.py, test_cli_ingest_gpu.py): the
acceptance rule of hga_count_add_file restated, the sequential reader as the oracle for the bytes, and the
three seeded file families (accepted FASTA, accepted 4-line FASTQ, refused)."""
import os
import random
import tempfile

EMPTY, FASTA, FASTQ, REFUSED = 0, 1, 2, 3


def getlines(data: bytes):
    """Lines as std::getline sees them: no extra empty line behind a final newline."""
    if not data:
        return []
    ls = data.split(b"\n")
    return ls[:-1] if data.endswith(b"\n") else ls


def expected_layout(data: bytes):
    """(layout, records, lines) by the rule in include/hga.h, written out line by line."""
    ls = getlines(data)
    first = next((i for i, l in enumerate(ls) if l), None)
    if first is None:
        return EMPTY, 0, len(ls)
    if ls[first][:1] == b">":
        return FASTA, sum(1 for l in ls if l[:1] == b">"), len(ls)
    ok = ls[first][:1] == b"@" and first == 0 and len(ls) % 4 == 0
    for r in range(0, len(ls) if ok else 0, 4):
        ok = ok and ls[r][:1] == b"@" and ls[r + 1][:1] != b"+" and ls[r + 2][:1] == b"+" and \
            len(ls[r + 1]) == len(ls[r + 3])
    return (FASTQ, len(ls) // 4, len(ls)) if ok else (REFUSED, 0, len(ls))


def oracle_stream(hga, data: bytes) -> bytes:
    """The sequential reader's stream of these bytes (hga.set_host_threads(1) is the caller's)."""
    with tempfile.NamedTemporaryFile(suffix=".reads", delete=False) as f:
        f.write(data)
    try:
        return hga.jf_stream(f.name)
    finally:
        os.unlink(f.name)


def _seq(rng, n, alphabet="ACGTACGTACGTNacgtn"):
    return "".join(rng.choices(alphabet, k=n))


def gen_fasta(rng, size):
    """Accepted FASTA of about `size` bytes: multi-line records, sequence lines starting with '@' / '+',
    empty lines, CR, empty records, optional leading empty lines and missing final newline."""
    out = ["\n" * rng.choice([0, 0, 1, 3])]
    n = len(out[0])
    while n < size or len(out) < 2:
        rec = [">" + _seq(rng, rng.choice([0, 1, 8, 30]), "abcdefgh 0123:/>@+")]
        for _ in range(rng.choice([0, 1, 1, 2, 5])):
            kind = rng.random()
            ln = _seq(rng, rng.choice([1, 2, 60, 61, 200]))
            if kind < 0.1:
                ln = ""
            elif kind < 0.2:
                ln = rng.choice("@+") + ln
            elif kind < 0.3:
                ln += "\r"
            rec.append(ln)
        text = "\n".join(rec) + "\n"
        out.append(text)
        n += len(text)
    data = "".join(out)
    tail = rng.random()
    if tail < 0.3:
        data = data[:-1]
    elif tail < 0.4:
        data += "\n"
    return data.encode()


def gen_fastq(rng, size, crlf=False):
    """Accepted 4-line FASTQ of about `size` bytes: quality lines starting with '@' / '+', empty sequences,
    optional missing final newline.  (No sequence line starts with '@': cut_records' rule.)"""
    out, n = [], 0
    while n < size or not out:
        ln = rng.choice([0, 1, 2, 35, 100, 151])
        seq = _seq(rng, ln)
        q = "".join(rng.choice("@+IJ#5") for _ in range(ln))
        eol = "\r\n" if crlf else "\n"
        text = "@" + _seq(rng, rng.choice([0, 5, 20]), "read/12 @+>") + eol + seq + eol + "+" + rng.choice(["", "x"]) + eol + q + eol
        out.append(text)
        n += len(text)
    data = "".join(out)
    if rng.random() < 0.3 and not data.endswith("\n\n"):   # (an empty last line would be lost with its newline)
        data = data[:-1]
    return data.encode()


DEFECTS = ["five", "lines", "plus", "qlen", "multi"]


def break_fastq(rng, data: bytes, where: str) -> bytes:
    """One defect in the first / last record of an accepted FASTQ file of records with non-empty sequences."""
    ls = getlines(data)
    return apply_defect(ls, 0 if where == "first" else len(ls) - 4, rng.choice(DEFECTS))


def apply_defect(ls, r, kind) -> bytes:
    ls = list(ls)
    if kind == "five":        # a 5-line record, and three lines more: the line count stays a multiple of 4
        ls[r + 3:r + 4] = [ls[r + 3], b"IIII", b"@x", b"A", b"+"]
    elif kind == "lines":     # line count not a multiple of 4
        ls.insert(r + 4, b"@tail")
    elif kind == "plus":      # sequence line starting with '+'
        ls[r + 1] = b"+" + ls[r + 1][1:]
    elif kind == "qlen":      # quality one byte longer
        ls[r + 3] = ls[r + 3] + b"I"
    elif kind == "multi":     # the sequence and the quality over two lines each; 8 lines where there were 4
        s, q = ls[r + 1], ls[r + 3]
        h = max(1, len(s) // 2)
        ls[r:r + 4] = [ls[r], s[:h], s[h:], ls[r + 2], q[:h], q[h:], b"@pad", b"A"]
    else:
        raise ValueError(kind)
    return b"\n".join(ls) + b"\n"


def plain_fastq(rng, size):
    """4-line FASTQ with non-empty sequences only (a base for the defects)."""
    out, n = [], 0
    while n < size:
        ln = rng.choice([4, 35, 100])
        text = f"@r{len(out)}\n{_seq(rng, ln, 'ACGT')}\n+\n{'I' * ln}\n"
        out.append(text)
        n += len(text)
    return "".join(out).encode()


def gen_refused(rng, size):
    kind = rng.random()
    if kind < 0.6:
        return break_fastq(rng, plain_fastq(rng, size), rng.choice(["first", "last"]))
    if kind < 0.8:
        return b"\n" + plain_fastq(rng, size)          # a leading empty line before '@'
    return _seq(rng, 10).encode() + b"\n" + gen_fasta(rng, size)   # first byte neither '>' nor '@'


FAMILIES = {"fasta": (gen_fasta, FASTA), "fastq": (gen_fastq, FASTQ), "refused": (gen_refused, REFUSED)}


SLACK = 1400   # a generator passes its size by less than one record and a defect


def fuzz_files(seed, count, max_size):
    """`count` (family, data) pairs, the families in turn, of at most max_size bytes."""
    rng = random.Random(seed)
    names = list(FAMILIES)
    out = []
    for i in range(count):
        fam = names[i % len(names)]
        size = rng.choice([rng.randint(1, 200), rng.randint(200, max_size // 4), rng.randint(max_size // 4, max_size)])
        data = FAMILIES[fam][0](rng, max(1, size - SLACK))
        assert len(data) <= max_size, (fam, len(data))
        out.append((fam, data))
    return out
