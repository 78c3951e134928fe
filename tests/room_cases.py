"""The retries of the read mapper's loop (stralg_amd/csrc/sx_map.hip, map_reads_loop): a batch whose
hits do not fit the room makes the room grow or is halved, and runs again.  SX_FLAG_SAM_ROOM_HITS (Context.set_sam_room_hits)
makes that happen on the fixtures, Context.map_stats() says that it did, and the text is compared with the reference mapper's
recorded output (best_cases.plain_of / want_of, sam_cases.check_case) -- never with a run of this library without the switch.
What the CPU-harness suite (tests/test_room_cpu.py) and the GPU suite (tests/test_gpu_room.py) share.  TEST INFRASTRUCTURE
ONLY.

The rooms, named by what they must provoke (check_stats):
  grow   a switch far above the need and batches of 8 reads: the first room is the guess of 4 hits a (read, record), and the
         batches that need more make it grow
  tight  a switch between the hits of the heaviest group and those of the whole call: batches are halved until they fit, and
         no group needs more than the room may hold
  lone   a switch below the hits of the heaviest group: that group is halved down to, and then gets whatever it needs
  one    a room of one hit: every batch is halved down to one group
A group is what a batch is halved in: a read (with both strands each strand is a read of its own), or, in best-stratum
mode on both strands, the two strands of a read.

The switches of tight and lone come from the recorded text.  A hit is an interval of the suffix array and an edit script;
it prints a line a row with its CIGAR.  So the distinct (RNAME, CIGAR) of a group's lines are a lower bound on its hits (a
CIGAR says M for a match and for a substitution: scripts that differ in a substituted letter print alike), and its lines are
an upper bound.  `lone` takes a third of the heaviest group's lower bound; `tight` takes the heaviest group's upper bound,
which must stay below the lower bound of the whole call.  At one edit a read of m symbols over s letters has 1 + m (s - 1) +
m + (m + 1) s scripts at most (none, a substitution, a symbol of the read skipped, a letter put in), a second upper bound:
the one that serves hg38/reads-100-10-0, where two reads have 7832 lines each.  The stats conditions are asserted, not
trusted.

One cell is not what the plain matrix says: best-stratum x grow on two-records-best.  The room's guess is 8 hits a read there
(two records) and no read of that fixture has more than 8 hits in its best stratum, so a batch of several reads can never
need more than the guess: the branch is out of reach by arithmetic.  hg38/reads-100-10-0 at k = 1 in best-stratum mode
(one record, a guess of 4 hits a read, 6 hits a read on average) takes that cell's place, one strand and both (BEST_GROW).

Nothing is cut on the CPU harness: the `one` rooms run all 240 reads."""
import best_cases as bc
from sam_cases import check_case, sam_cases
from strand_cases import fastq_reads

ROOMS = ("grow", "tight", "lone", "one")
FAR_ABOVE = 1 << 20
FORMS = [dict(), dict(compact=True), dict(compact=True, sa_sample=32), dict(compact=True, packed=True, sa_sample=32)]
FORM_IDS = ["full", "compact", "sampled", "packed-sampled"]

_CASES = {}


def best_case(name="two-records-best"):
    if "best" not in _CASES:
        _CASES["best"] = bc.best_cases()
    return _CASES["best"][name]


def sam_case(name="hg38/reads-100-10-0/k1"):
    if "sam" not in _CASES:
        _CASES["sam"] = sam_cases()
    return _CASES["sam"][name]


def text_of(case, k, both, best):
    """the recorded text of a call on one of best_cases' cases"""
    return (bc.want_of if best else bc.plain_of)(case, k, both)


def group_lines(text, whole_reads):
    """group -> [(FLAG, RNAME, CIGAR) of its lines], in file order, over the groups that have lines; a group: a (QNAME, FLAG),
    or the QNAME where whole_reads (both strands of a read are one group)"""
    per = {}
    for line in text.split(b"\n")[:-1]:
        f = line.split(b"\t")
        per.setdefault(f[0] if whole_reads else (f[0], f[1]), []).append((f[1], f[2], f[5]))
    return per


def group_hits(text, whole_reads):
    """[a lower bound on a group's hits: the distinct (FLAG, RNAME, CIGAR) of its lines]"""
    return [len(set(v)) for v in group_lines(text, whole_reads).values()]


def scripts_at_one_edit(m, letters):
    return 1 + m * (letters - 1) + m + (m + 1) * letters


def switch_of(room, text, whole_reads=False, most=None):
    """the value of SX_FLAG_SAM_ROOM_HITS that makes `room` of a call whose recorded text is `text`; most: an upper bound on
    the hits of a read from elsewhere"""
    hits = group_hits(text, whole_reads)
    heaviest, total = max(hits), sum(hits)
    if room == "grow":
        return FAR_ABOVE
    if room == "tight":
        upper = max(len(v) for v in group_lines(text, whole_reads).values())
        if most is not None:
            upper = min(upper, most * (2 if whole_reads else 1))
        assert heaviest <= upper < total
        return upper
    if room == "lone":
        assert heaviest >= 3
        return heaviest // 3
    assert room == "one"
    return 1


def tight_switch_of_batches(fastq, text, groups):
    """the tight room of a best-stratum call on both strands whose batches hold `groups` reads' strands: between the
    heaviest read and the heaviest batch (the batches of the first pass start at multiples of `groups` reads), both by
    their lower bounds: the fixture leaves no room for more (a read of 8 to 16 hits, a batch of 15 at least)"""
    per = group_lines(text, True)
    hits = [len(set(per.get(r[0], ()))) for r in fastq_reads(fastq)]
    heaviest, batch = max(hits), max(sum(hits[i:i + groups]) for i in range(0, len(hits), groups))
    switch = (heaviest + batch) // 2
    assert heaviest <= switch < batch
    return switch


def check_stats(room, st, switch, g=1):
    """what the room must have provoked; g: the reads of a group"""
    assert st["retries"] == st["room_grown"] + st["lone_grown"] + st["halved"], st
    assert st["batches"] >= 1 and st["room_first"] <= st["room_final"] and st["batch_final"] <= st["batch_first"], st
    assert st["batch_final"] % g == 0, st
    if room == "grow":
        assert st["room_grown"] >= 1 and st["halved"] == 0 and st["room_final"] <= switch, st
    elif room == "tight":
        assert st["halved"] >= 1 and st["lone_grown"] == 0, st
    elif room == "lone":
        assert st["halved"] >= 1 and st["lone_grown"] >= 1 and st["room_final"] > switch, st
    else:
        assert room == "one"
        assert st["batch_final"] == g and st["halved"] >= 1, st


def check_untouched(st):
    """a call with the switch back at 0: nothing is retried, the room is what the memory gives"""
    assert st["retries"] == 0 and st["halved"] == 0 and st["room_first"] >= 1 << 16 and st["room_final"] == st["room_first"], st


def with_room(ctx, switch, call, batch=0, window=0, chunk_rows=0):
    """(what call() returns, the stats of its last mapping call) with the switches set, and every switch back at 0 behind it"""
    ctx.set_sam_room_hits(switch)
    ctx.set_sam_batch_reads(batch)
    ctx.set_sam_window_bytes(window)
    ctx.set_locate_chunk_rows(chunk_rows)
    try:
        got = call()
        return got, ctx.map_stats()
    finally:
        ctx.set_sam_room_hits(0)
        ctx.set_sam_batch_reads(0)
        ctx.set_sam_window_bytes(0)
        ctx.set_locate_chunk_rows(0)


def stream(ctx, records, fastq, k, both=False, best=False):
    """the text of sx_map_reads_stream on host tables"""
    chunks = []
    ctx.map_reads_stream(records, fastq, k, chunks.append, both_strands=both, best=best)
    return b"".join(chunks)


# ---- the matrix -------------------------------------------------------------------------------------------------------------
MODES = [(best, both) for best in (False, True) for both in (False, True)]
MODE_IDS = ["%s-%s" % ("best" if best else "plain", "both" if both else "one") for best, both in MODES]
BEST_GROW = ("hg38/reads-100-10-0", 1)  # (see above)


def check_stream_room(ctx, records_of, room, best, both, k=2):
    """sx_map_reads_stream on two-records-best at k edits in one of the rooms.  records_of(fasta) -> [(name, BwtTable)]"""
    name = "two-records-best"
    if room == "grow" and best:
        name, k = BEST_GROW
    c = best_case(name)
    want = text_of(c, k, both, best)
    g = 2 if best and both else 1
    switch = switch_of(room, want, g == 2)
    got, st = with_room(ctx, switch, lambda: stream(ctx, records_of(c["fasta"]), c["fastq"], k, both, best), batch=8 if room == "grow" else 0)
    bc.check_text(got, want)
    check_stats(room, st, switch, g)
    return st


def check_interleaved(ctx, records_of):
    """best-stratum on both strands, the batch switch at 7 (the plan makes it 8: whole groups), windows of 1000 bytes, a
    tight room: rooms, batches and windows interleave"""
    c = best_case()
    want = text_of(c, 2, True, True)
    switch = tight_switch_of_batches(c["fastq"], want, 4)
    chunks = []

    def call():
        ctx.map_reads_stream(records_of(c["fasta"]), c["fastq"], 2, chunks.append, both_strands=True, best=True)

    _, st = with_room(ctx, switch, call, batch=7, window=1000)
    assert max(len(x) for x in chunks) <= 1008
    bc.check_text(b"".join(chunks), want)
    assert st["batch_first"] == 8
    check_stats("tight", st, switch, 2)
    return st


def check_one_record(ctx, records_of, best):
    """one record, wide intervals: hg38/reads-100-10-0 at one edit in a tight room"""
    if best:
        c = best_case("hg38/reads-100-10-0")
        want = text_of(c, 1, False, True)
    else:
        c = sam_case()
        want = c["sam"]
    reads = fastq_reads(c["fastq"])
    letters = len(set(b"".join(r[1] for r in reads)) | set(b"ACGT"))
    switch = switch_of("tight", want, most=scripts_at_one_edit(max(len(r[1]) for r in reads), letters))
    got, st = with_room(ctx, switch, lambda: stream(ctx, records_of(c["fasta"]), c["fastq"], 1, False, best))
    bc.check_text(got, want)
    if not best:
        check_case(c, got)
    check_stats("tight", st, switch)
    return st


def check_index_form(ctx, Index, form, best):
    """Index.from_fasta in one form, both strands at two edits in the lone room; the sampled forms locate in runs of 64 rows.
    The room that grew for a lone group makes the merged hits' buffers be taken again, the lines' offsets with them"""
    c = best_case()
    want = text_of(c, 2, True, best)
    g = 2 if best else 1
    switch = switch_of("lone", want, g == 2)
    rows = 64 if form.get("sa_sample") else 0
    with Index.from_fasta(c["fasta"], ctx=ctx, **form) as idx:
        got, st = with_room(ctx, switch, lambda: idx.map_reads(c["fastq"], 2, both_strands=True, best=best), chunk_rows=rows)
        bc.check_text(got, want)
        check_stats("lone", st, switch, g)
    return st


def check_discard_and_back(ctx, Index, form):
    """map_reads_discard in the lone room: the sink does not see the text, so its bytes are counted against the recorded
    text's; then the same context and index with the switch back at 0: the recorded text, nothing retried, the room what the
    memory gives (the counters and the room are a call's own)"""
    c = best_case()
    want = text_of(c, 2, True, False)
    switch = switch_of("lone", want)
    rows = 64 if form.get("sa_sample") else 0
    with Index.from_fasta(c["fasta"], ctx=ctx, **form) as idx:
        seen, st = with_room(ctx, switch, lambda: idx.map_reads_discard(c["fastq"], 2, both_strands=True), chunk_rows=rows)
        assert sum(n for _, n in seen) == len(want)
        check_stats("lone", st, switch)
        got, st = with_room(ctx, switch, lambda: idx.map_reads(c["fastq"], 2, both_strands=True), chunk_rows=rows)
        bc.check_text(got, want)
        assert got.count(b"\n") == want.count(b"\n")
        check_stats("lone", st, switch)
        bc.check_text(idx.map_reads(c["fastq"], 2, both_strands=True), want)
        check_untouched(ctx.map_stats())
        bc.check_text(idx.map_reads(c["fastq"], 2, both_strands=True, best=True), text_of(c, 2, True, True))
        check_untouched(ctx.map_stats())
    return st


def check_no_edits(ctx, records_of, best, both):
    """k = 0 in a room of one hit: most reads have no hit, so batches without hits pass between the halvings"""
    c = best_case()
    want = text_of(c, 0, both, best)
    names = [r[0] for r in fastq_reads(c["fastq"])]
    assert len({l.split(b"\t", 1)[0] for l in want.split(b"\n")[:-1]}) < len(names) // 2
    g = 2 if best and both else 1
    got, st = with_room(ctx, 1, lambda: stream(ctx, records_of(c["fasta"]), c["fastq"], 0, both, best))
    bc.check_text(got, want)
    check_stats("one", st, 1, g)
    return st
