"""FASTQ images for sx_fastq_index_dev (sx_fastq.hip), shared by the CPU-harness suite (tests/test_index_cpu.py) and the
GPU suite (tests/test_gpu_fastq.py), and the three parties every image is put to: fastq_reference below (Python, written
from the contract in include/stralg_amd.h), the host's sx_fastq_index and the device's sx_fastq_index_dev.  `mem` is one
of the two objects of tests/device_memory.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from stralg_amd import api

TILE = 4096  # bytes of the image a workgroup of the indexer's passes takes (kFqTile)


# ---- the contract, restated ----------------------------------------------------------------------------------------------
def fastq_reference(data):
    """The contract of sx_fastq (include/stralg_amd.h): None for a malformed image, else (names, seqs, quals, name_off,
    seq_off, qual_off) -- three byte strings and three offset lists of count + 1 entries."""
    if b"\0" in data:
        return None
    lines = data.split(b"\n")
    if lines[-1] == b"":  # (the piece behind a final newline; an empty image is this piece alone: zero records)
        lines.pop()
    if len(lines) % 4:
        return None
    out, off = [[], [], []], [[0], [0], [0]]
    for r in range(0, len(lines), 4):
        first, second, third, fourth = lines[r:r + 4]
        if not 2 <= len(first) <= 2046 or not second or not fourth or max(len(second), len(third), len(fourth)) >= 2047:
            return None
        for k, field in enumerate((first[1:], second, fourth)):  # (the first byte of a record is dropped whatever it is)
            out[k].append(field)
            off[k].append(off[k][-1] + len(field))
    return b"".join(out[0]), b"".join(out[1]), b"".join(out[2]), off[0], off[1], off[2]


def host_result(ctx, data):
    try:
        return ctx.fastq_index(data), None
    except api.StralgAmdError as e:
        return None, str(e).rsplit("code ", 1)[1].split(":")[0].split()[0]


def dev_result(ctx, mem, data, shift=0):
    d_image = mem.to_dev(data, shift)
    mem.sync()
    try:
        arrays, count = ctx.fastq_index_dev(d_image, len(data))
        return (arrays, count), None
    except api.StralgAmdError as e:
        return None, str(e).split("code ", 1)[1].split(":")[0].split()[0]


def agree(ctx, mem, data, shift=0, expect=None):
    """the three parties on one image: the same verdict, and inside the contract the same six arrays; returns the
    error code (None inside the contract)"""
    ref = fastq_reference(data)
    want, werr = host_result(ctx, data)
    got, gerr = dev_result(ctx, mem, data, shift)
    assert werr == gerr, (data[:80], werr, gerr)
    assert werr == (None if ref is not None else "-4"), (data[:80], len(data), werr, "the contract's restatement differs")
    if expect is not None:
        assert (werr is None) == expect, (data[:80], werr)
    if want is not None:
        arrays, count = got
        assert count == want[1].size - 1
        for g, w in zip(arrays, want):
            assert g.dtype == w.dtype and g.size == w.size and (g == w).all(), data[:80]
        names, seqs, quals, name_off, seq_off, qual_off = ref
        for k, (text, off) in enumerate(((names, name_off), (seqs, seq_off), (quals, qual_off))):
            assert arrays[2 * k].tobytes() == text, (data[:80], shift, k)
            assert arrays[2 * k + 1].tolist() == off, (data[:80], shift, k)
    return werr


def check_image(ctx, mem, case):
    """case: (image bytes, shift of its first byte off a 16-byte boundary, inside the contract or not or None)"""
    data, shift, expect = case
    return agree(ctx, mem, data, shift, expect)


def check_deterministic(ctx, mem, case):
    """the indexer twice on the same device image: the same bytes (and the host's)"""
    data, shift, _ = case
    d_image = mem.to_dev(data, shift)
    mem.sync()
    first, count = ctx.fastq_index_dev(d_image, len(data))
    again, count2 = ctx.fastq_index_dev(d_image, len(data))
    assert count == count2 and all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    assert all(a.tobytes() == w.tobytes() for a, w in zip(first, ctx.fastq_index(data)))


# ---- the images ------------------------------------------------------------------------------------------------------------
IN_CONTRACT = b"@r0 desc x\nCC\n+\n~~\n@r1\nAAA\n+r1 again\nIII\n@@\n@\n+\n+\n@last\tname\nNN\n\n##"
LONGEST = b"@" + b"n" * 2045 + b"\n" + b"A" * 2046 + b"\n+\n" + b"I" * 2046

OUT_OF_CONTRACT = [  # the images of test_sam_cpu.test_fastq_index_out_of_contract
    b"@" + b"n" * 2046 + b"\nA\n+\nI\n",
    b"@r\n" + b"A" * 2047 + b"\n+\n" + b"I" * 2047 + b"\n",
    b"@\nA\n+\nI\n",
    b"@r\n\n+\nI\n",
    b"@r\nA\n+\n\n",
    b"@r\nA\n+\n",
    b"@r\nA\n+",
    b"@r\nA\n",
    b"@r\n",
    b"@r\nA\n+\nI\n\n",
    b"\n@r\nA\n+\nI\n",
    b"@r\nA\0\n+\nI\n",
]


def fixture_images(cases):
    """every distinct FASTQ image of tests/golden/golden_sam.npz, as it is and without its final newline at shift 3"""
    seen, out = set(), []
    for c in cases.values():
        if c["fastq"] not in seen:
            seen.add(c["fastq"])
            out.append((c["fastq"], 0, True))
            out.append((c["fastq"].rstrip(b"\n"), 3, True))
    return out


def in_contract_images():
    return [(data, shift, True) for data in (IN_CONTRACT, IN_CONTRACT + b"\n", b"", LONGEST, LONGEST + b"\n")
            for shift in (0, 1, 4)]


def check_in_contract_fields(ctx, mem):
    d_image = mem.to_dev(IN_CONTRACT)
    mem.sync()
    (names, no, seqs, so, quals, qo), count = ctx.fastq_index_dev(d_image, len(IN_CONTRACT))
    split = lambda d, o: [d[o[i]:o[i + 1]].tobytes() for i in range(o.size - 1)]
    assert count == 4 and split(names, no) == [b"r0 desc x", b"r1", b"@", b"last\tname"]
    assert split(seqs, so) == [b"CC", b"AAA", b"@", b"NN"] and split(quals, qo) == [b"~~", b"III", b"+", b"##"]


def random_record(rng, edge):
    """four lines of a record inside the contract; `edge`: line lengths near the limit"""
    alphabet = np.frombuffer(b"ACGTN@+ \t~!IJ>", np.uint8)

    def line(lo):
        n = int(rng.integers(2040, 2047)) if edge and rng.integers(0, 3) == 0 else int(rng.integers(lo, 40))
        return rng.choice(alphabet, n).tobytes()

    return [line(2), line(1), line(0), line(1)]


def image_of(records, final_newline):
    return b"\n".join(b"\n".join(r) for r in records) + (b"\n" if final_newline and records else b"")


FILLER = [b"@" + b"n" * 14, b"A" * 15, b"+" + b"x" * 14, b"I" * 15]  # 64 bytes with its newlines


def generated_images():
    """random records, some with lines near the limit and some shifted; lengths around multiples of 16 and of the tile;
    a newline as the last byte of a tile, the first byte of the next, and the one behind it"""
    out = []
    rng = np.random.default_rng(11)
    for k in range(60):
        recs = [random_record(rng, edge=k % 3 == 0) for _ in range(int(rng.integers(1, 30)))]
        out.append((image_of(recs, k % 2 == 0), int(rng.integers(0, 16)) if k % 4 == 0 else 0, True))
    # lengths around multiples of 16 and of the 4096-byte tile: the last record's quality line is stretched or cut
    base = [random_record(rng, False) for _ in range(150)]
    for target in (4096, 8192, 4096 * 3):
        for delta in (-17, -16, -15, -2, -1, 0, 1, 2, 15, 16, 17):
            for final in (False, True):
                recs, size = [], 0
                for r in base:
                    recs.append(list(r))
                    size = len(image_of(recs, final))
                    if size >= target + delta - 30:
                        break
                pad = target + delta - size
                if pad >= 0:
                    recs[-1][3] += b"I" * pad
                else:
                    recs[-2][3] = recs[-2][3] + b"I" * 60
                    recs[-1][3] = (recs[-1][3] + b"I" * 60)[:max(1, len(recs[-1][3]) + 60 + pad)]
                out.append((image_of(recs, final), 0, True))
    # a newline as the last byte of a tile, the first byte of the next, and the one behind it
    for at in (4095, 4096, 4097):
        seq = b"C" * (at - 63 * 64 - 3)
        data = image_of([FILLER] * 63 + [[b"@n", seq, b"+", b"#" * len(seq)]] + [FILLER] * 70, True)
        assert data[at] == 10 and data[at - 1] == ord("C")
        out.append((data, 0, True))
    return out


DEFECTS = ["long_line", "empty_name", "one_byte_name", "empty_seq", "empty_qual", "cut", "blank_before", "blank_between",
           "blank_behind", "nul", "none"]


def with_defect(rng, lines, at, defect, final):
    """the lines of well-formed records with one defect at record `at` (or at the image's ends): (lines, final newline)"""
    if defect == "long_line":
        lines[4 * at + int(rng.integers(0, 4))] = b"@" + b"x" * int(rng.integers(2046, 2050))
    elif defect == "empty_name":
        lines[4 * at] = b""
    elif defect == "one_byte_name":
        lines[4 * at] = b"@"
    elif defect == "empty_seq":
        lines[4 * at + 1] = b""
    elif defect == "empty_qual":
        lines[4 * at + 3] = b""
    elif defect == "cut":
        lines = lines[:len(lines) - int(rng.integers(1, 4))]
    elif defect == "blank_before":
        lines.insert(0, b"")
    elif defect == "blank_between":
        lines.insert(4 * at, b"")
    elif defect == "blank_behind":
        lines.append(b"")
        final = True
    elif defect == "nul":
        j = 4 * at + int(rng.integers(0, 4))
        lines[j] = lines[j] + b"\0" + lines[j]
    return lines, final


def soups():
    """330 images of random records with one defect each: (defect, image)"""
    rng = np.random.default_rng(12)
    out = []
    for k in range(330):
        recs = [random_record(rng, edge=False) for _ in range(int(rng.integers(1, 120)))]
        at = int(rng.integers(0, len(recs)))
        defect = DEFECTS[k % len(DEFECTS)]
        lines = [l for r in recs for l in r]
        final = bool(rng.integers(0, 2))
        lines, final = with_defect(rng, lines, at, defect, final)
        out.append((defect, b"\n".join(lines) + (b"\n" if final else b"")))
    return out


def check_defects(ctx, mem, cases):
    """cases: (defect, image); every defect but "none" is malformed for all three parties, "none" is not"""
    seen = {}
    for defect, data in cases:
        err = agree(ctx, mem, data)
        seen.setdefault(defect, set()).add(err)
    # (an empty quality line at the very end without a final newline reads as a record cut off: malformed either way)
    assert seen.pop("none") == {None}
    assert all(v == {"-4"} for v in seen.values()), seen
    assert len(seen) == len(DEFECTS) - 1


# ---- images aimed at the passes' tiles (4096 bytes a workgroup, 16 bytes a lane) --------------------------------------------
def line_at_a_tile_edge(role, tile, ends):
    """an image whose line of role `role` (0 name .. 3 quality) of one record starts exactly at byte 4096 x tile (the
    newline in front of it is the previous tile's last byte), or, with `ends`, has its last byte in front of that place
    and its newline exactly there"""
    at = TILE * tile
    lines = [b"@n", b"ACG", b"+", b"#!#"]
    room = 128 if (role or ends) else 0
    if room:
        j = role if ends else role - 1  # the line that is stretched: through its newline the record has `want` bytes
        want = room + (1 if ends else 0)
        used = sum(len(l) + 1 for l in lines[:j + 1])
        lines[j] = lines[j] + (b"x" if j != 1 else b"T") * (want - used)
    data = image_of([FILLER] * ((at - room) // 64) + [lines] + [FILLER] * 70, True)
    start = at - room + sum(len(l) + 1 for l in lines[:role])
    if ends:
        assert data[at] == 10 and start + len(lines[role]) == at
    else:
        assert start == at and data[at - 1] == 10 and data[at] == lines[role][0]
    return data


def line_role_edge_images():
    return [(line_at_a_tile_edge(role, tile, ends), 0, True) for role in range(4) for tile in (1, 2) for ends in (False, True)]


def long_line_images():
    """a line of 2046 bytes across a tile boundary in every role (the line the next tile's first byte lies in starts in
    the tile before), and records of two such lines, so that tiles hold one or two newlines"""
    out = []
    for role in range(4):
        for lead in (33, 40, 63):  # the line starts 1984, 1536 and 64 bytes or so in front of the boundary
            lines = [b"@n", b"ACG", b"+", b"#!#"]
            lines[role] = lines[role][:1] + b"L" * 2045
            data = image_of([FILLER] * lead + [lines] + [FILLER] * 70, role % 2 == 0)
            out.append((data, 0, True))
    two = [b"@r", b"G" * 2046, b"+", b"J" * 2046]
    out.append((image_of([two] * 5, True), 0, True))
    out.append((image_of([FILLER] + [two] * 4 + [FILLER], False), 5, True))
    return out


SHORTEST = [b"@a", b"A", b"", b"I"]  # 9 bytes with its newlines


def dense_tile_images():
    """a tile full of the shortest legal records (about 1820 line starts in a workgroup's table) next to tiles of few
    newlines (lines of 2046 bytes) and, outside the contract, next to a tile without any newline (a line of 5000 bytes)"""
    two = [b"@r", b"G" * 2046, b"+", b"J" * 2046]
    out = [(image_of([SHORTEST] * 1000, True), 0, True),
           (image_of([SHORTEST] * 456 + [two] * 2 + [SHORTEST] * 460, True), 0, True),
           (image_of([two] + [SHORTEST] * 910 + [two], False), 7, True),
           (image_of([SHORTEST] * 455 + [[b"@r", b"G" * 5000, b"+", b"J"]] + [SHORTEST] * 455, True), 0, False),
           (image_of([SHORTEST] * 455 + [[b"@r", b"G", b"+" * 5000, b"J"]] + [SHORTEST] * 455, True), 0, False)]
    return out


def image_of_length(n, final):
    """64-byte records and a last one whose quality line brings the image to n bytes exactly"""
    k = (n - 12) // 64
    rest = n - 64 * k  # the last record's bytes: "@n\nAC\n+\n" (8), the quality line, and the final newline if any
    data = image_of([FILLER] * k + [[b"@n", b"AC", b"+", b"I" * (rest - 8 - (1 if final else 0))]], final)
    assert len(data) == n
    return data


def shifted_tile_multiple_images():
    """every shift off a 16-byte boundary with an image of a multiple of 4096 bytes, one more and one less"""
    return [(image_of_length(TILE * tiles + delta, final), shift, True)
            for shift in range(16) for tiles, delta, final in ((2, -1, True), (2, 0, False), (2, 1, True), (1, 0, True), (3, 0, True),
                                                               (3, 1, False), (3, -1, False))]


def defects_at_tile_edges():
    """every defect in the last record of a tile, the first of the next, and the last record of an image of several
    tiles (64-byte records: record 63 ends tile 0): (defect, image)"""
    rng = np.random.default_rng(13)
    out = []
    for defect in DEFECTS:
        for at in (63, 64, 99):
            for final in (False, True):
                lines = [l for _ in range(100) for l in FILLER]
                lines, fin = with_defect(rng, lines, at, defect, final)
                out.append((defect, b"\n".join(lines) + (b"\n" if fin else b"")))
    return out


def determinism_images():
    rng = np.random.default_rng(14)
    out = []
    for k, shift in enumerate((0, 5, 12)):
        recs = [random_record(rng, edge=k == 1) for _ in range(120 + 200 * k)]
        out.append((image_of(recs, k != 2), shift, True))
    return out
