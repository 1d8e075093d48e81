"""Cases and numpy models for the routines the text tools share: the grouped
wave copies of csrc/wavecopy.h (piece_group_copy through magot_debug_piece_copy,
span_group_copy through magot_copy_segments and magot_debug_text_assembly) and
the line modes of csrc/textindex.hip (magot_debug_text_lines).

The models are slicing and concatenation.  The builders are deterministic
(seeded random.Random / numpy.random.RandomState): random source bytes, and an
output buffer prefilled with a position-dependent pattern that ends in GUARD
bytes no piece covers, so that a comparison of the whole buffer sees a chunk
stored over a neighbour, over a gap or over the end.

A class of a copied piece is (source offset mod 16, destination offset mod 16,
length).  With the lengths 0..49 every destination phase meets 0, 1, 2 and 3
whole 16-byte chunks with every head and tail length, and both sides of the
`a16 + 16 <= e` threshold.  deal() and rounds() restate how the routines split
a piece into whole chunks and byte-stored bytes and how many rounds of its two
loops a group of 16 takes; they serve the coverage assertions of
test_wavecopy_expect.py, not the expected bytes.  Nothing here imports the
code under test."""

import random

import numpy as np

GUARD = 64
GROUP = 16               # pieces per wave (kSpanGroup, kFaGroup, kRnGroup)
CHUNK_ROUND = 64 * 4     # whole chunks per round of a wave's chunk loop (64 x kSpanUnroll)
BYTE_ROUND = 64 * 8      # byte-stored bytes per round of its byte loop (64 x kSpanBytes)
LENS = tuple(range(50))
TRIPLES = tuple((s, d, n) for s in range(16) for d in range(16) for n in LENS)
GROUP_SIZES = (1, 15, 16, 17, 63, 64, 65)  # one wave; one workgroup of four; the next workgroup
NO_RECORD = 0xFFFFFFFF
UNIT_DTYPE = np.dtype([('text_off', '<u8'), ('text_len', '<u4'), ('rec', '<u4')])
LF, CR, X = 10, 13, ord('X')
NO_STRAY = 2 ** 64 - 1


def pattern(n):
    """n bytes that depend on their position"""
    i = np.arange(n, dtype=np.uint64)
    mixed = (i * np.uint64(131) + np.uint64(7)) ^ (i >> np.uint64(8))
    return (mixed & np.uint64(255)).astype(np.uint8)


def noise(seed, n, avoid=None):
    """n random bytes, none of them `avoid`"""
    b = np.random.RandomState(seed).randint(0, 256, size=n).astype(np.uint8)
    if avoid is not None:
        b[b == avoid] = avoid ^ 0x20
    return b


def place(lens, phases, order, gap):
    """(offsets, bytes used): piece k at an offset of phase phases[k] mod 16,
    the pieces laid out in `order` with at least `gap` bytes between neighbours
    and before the first"""
    off, at = [0] * len(lens), 0
    for k in order:
        at += gap
        at += (phases[k] - at) % 16
        off[k] = at
        at += lens[k]
    return off, at


def deal(o, te, e):
    """(whole chunks, byte-stored bytes) of the output piece [o, e) whose
    vector-copied part starts at te (o for a piece without a text part)"""
    a16 = (te + 15) & ~15
    if a16 + 16 <= e:
        g = e & ~15
        return (g - a16) >> 4, (a16 - o) + (e - g)
    return 0, e - o


def rounds(pieces):
    """[(chunk-loop rounds, byte-loop rounds)] of each group of GROUP
    consecutive pieces (o, te, e)"""
    out = []
    for k in range(0, len(pieces), GROUP):
        c = [deal(*p) for p in pieces[k:k + GROUP]]
        nf, nb = sum(x[0] for x in c), sum(x[1] for x in c)
        out.append((-(-nf // CHUNK_ROUND), -(-nb // BYTE_ROUND)))
    return out


def shuffled(seq, rnd):
    seq = list(seq)
    rnd.shuffle(seq)
    return seq


# ---------------------------------------------------------------------------
# lengths and phases shared by the three copies
# ---------------------------------------------------------------------------

def shape_lens():
    """{name: lengths} of the group shapes: the sizes around a wave and a
    workgroup, a group of empty pieces only, and empty pieces first and last in
    a group (ties in the inclusive counts the lanes are dealt by)"""
    rnd = random.Random(4)
    shapes = {'n%d' % n: [rnd.choice(LENS) for _ in range(n)] for n in GROUP_SIZES}
    some = lambda n: [rnd.randint(1, 49) for _ in range(n)]
    shapes['zero_group'] = some(16) + [0] * 16 + some(16)
    shapes['zero_edges'] = ([0] + some(14) + [0] +                      # first and last
                            [0, 0] + some(5) + [0, 0, 0] + some(4) + [0, 0] +  # runs of them
                            some(15) + [0] +                            # last only
                            [0] + some(3))                              # first, in a short group
    return shapes


# (index in its group, source phase, destination phase, length): the chunk loop's
# second round begins behind 256 whole chunks, its third behind 512
LONG_PIECES = ((5, 3, 9, 4200), (11, 13, 7, 8400))


def loop_specs(rnd):
    """[(source phase, destination phase or None, length)]: a group of tiny
    pieces, a group with one piece of 4,200 bytes, a group with one of 8,400"""
    specs = [(rnd.randrange(16), None, rnd.randint(0, 20)) for _ in range(3 * GROUP)]
    for g, (k, s, d, n) in enumerate(LONG_PIECES):
        specs[GROUP * (g + 1) + k] = (s, d, n)
    return specs


# ---------------------------------------------------------------------------
# piece_group_copy
# ---------------------------------------------------------------------------

class PieceCase(object):
    """out[dst[k]:dst[k] + len[k]] = base[src[k]:src[k] + len[k]]"""

    def __init__(self, base, src, dst, length, out):
        self.base = base
        self.src = np.asarray(src, dtype=np.uint64)
        self.dst = np.asarray(dst, dtype=np.uint64)
        self.len = np.asarray(length, dtype=np.uint32)
        self.out = out

    def model(self):
        want = self.out.copy()
        for s, d, n in zip(self.src.tolist(), self.dst.tolist(), self.len.tolist()):
            want[d:d + n] = self.base[s:s + n]
        return want

    def triples(self):
        return set(zip((self.src % 16).tolist(), (self.dst % 16).tolist(), self.len.tolist()))

    def spans(self):
        return [(d, d, d + n) for d, n in zip(self.dst.tolist(), self.len.tolist())]


def piece_case(specs, seed):
    """Pieces (source phase, destination phase or None, length), in table
    order; sources and destinations are laid out in two other orders, the
    destinations with at least one untouched byte between neighbours."""
    rnd = random.Random(seed)
    n = len(specs)
    lens = [p[2] for p in specs]
    dph = [rnd.randrange(16) if p[1] is None else p[1] for p in specs]
    src, src_used = place(lens, [p[0] for p in specs], shuffled(range(n), rnd), 0)
    dst, dst_used = place(lens, dph, shuffled(range(n), rnd), 1)
    return PieceCase(noise(seed, src_used + 1), src, dst, lens, pattern(dst_used + 1 + GUARD))


def piece_every_class():
    return piece_case(shuffled(TRIPLES, random.Random(1)), 1)


def piece_shapes():
    rnd = random.Random(5)
    cases = {name: piece_case([(rnd.randrange(16), None, n) for n in lens], 50 + i)
             for i, (name, lens) in enumerate(sorted(shape_lens().items()))}
    cases['n0'] = PieceCase(noise(9, 64), [], [], [], pattern(200))
    return cases


def piece_loops():
    return piece_case(loop_specs(random.Random(6)), 6)


# ---------------------------------------------------------------------------
# span_group_copy without text parts (magot_copy_segments)
# ---------------------------------------------------------------------------

class SegmentCase(object):
    """dst[dst_off[i]:dst_off[i + 1]] = src[src_off[i]:...]; dst_off is a prefix table"""

    def __init__(self, src, src_off, dst_off, dst):
        self.src = src
        self.src_off = np.asarray(src_off, dtype=np.uint64)
        self.dst_off = np.asarray(dst_off, dtype=np.uint64)
        self.dst = dst

    def model(self):
        want = self.dst.copy()
        do = self.dst_off.tolist()
        for i, s in enumerate(self.src_off.tolist()):
            want[do[i]:do[i + 1]] = self.src[s:s + do[i + 1] - do[i]]
        return want

    def triples(self):
        lens = np.diff(self.dst_off)
        return set(zip((self.src_off % 16).tolist(), (self.dst_off[:-1] % 16).tolist(),
                       lens.tolist()))

    def spans(self):
        do = self.dst_off.tolist()
        return [(do[i], do[i], do[i + 1]) for i in range(len(do) - 1)]


def segment_case(specs, start, seed):
    """Segments (source phase, destination phase or None, length) one behind
    the other from dst[start]; before a piece with a destination phase, a filler
    segment (an ordinary one) brings the destination to that phase."""
    rnd = random.Random(seed)
    phases, lens = [], []
    at = start
    for s, d, n in specs:
        fill = 0 if d is None else (d - at) % 16
        if fill:
            phases.append(rnd.randrange(16))
            lens.append(fill)
        phases.append(s)
        lens.append(n)
        at += fill + n
    src_off, used = place(lens, phases, shuffled(range(len(lens)), rnd), 0)
    dst_off = np.cumsum([start] + lens)
    return SegmentCase(noise(seed, used + 1), src_off, dst_off, pattern(at + GUARD))


SEGMENT_START = 5


def segment_every_class():
    return segment_case(shuffled(TRIPLES, random.Random(2)), SEGMENT_START, 2)


def segment_shapes():
    rnd = random.Random(7)
    return {name: segment_case([(rnd.randrange(16), None, n) for n in lens], 1 + 3 * i, 70 + i)
            for i, (name, lens) in enumerate(sorted(shape_lens().items()))}


def segment_loops():
    return segment_case(loop_specs(random.Random(8)), 11, 8)


# ---------------------------------------------------------------------------
# span_group_copy with text parts (magot_debug_text_assembly)
# ---------------------------------------------------------------------------

class AssemblyCase(object):
    """Unit i: text[text_off:text_off + text_len], then the payload
    pay[s:e] of record rec (s, e = rspan[2 rec], rspan[2 rec + 1]) unless rec
    is NO_RECORD; with `protein` a payload that begins with X loses that byte."""

    def __init__(self, units, text, rspan, pay, out):
        self.units, self.text, self.pay, self.out = units, text, pay, out
        self.rspan = np.asarray(rspan, dtype=np.uint64)

    def walk(self, protein):
        """per unit (o, te, e, payload start in pay or None, whether an X was
        trimmed): its output range, where its payload starts in it"""
        rows, at = [], 0
        span = self.rspan.tolist()
        for off, tl, rec in self.units.tolist():
            te, s, trimmed = at + tl, None, False
            e = te
            if rec != NO_RECORD:
                s, end = span[2 * rec], span[2 * rec + 1]
                trimmed = bool(protein and end > s and self.pay[s] == X)
                s += trimmed
                e = te + end - s
            rows.append((at, te, e, s, trimmed))
            at = e
        return rows

    def model(self, protein):
        """(the whole output buffer, the text's length)"""
        parts = []
        for (off, tl, rec), (o, te, e, s, _) in zip(self.units.tolist(), self.walk(protein)):
            parts.append(self.text[off:off + tl])
            if s is not None:
                parts.append(self.pay[s:s + e - te])
        body = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
        want = self.out.copy()
        want[:len(body)] = body
        return want, len(body)

    def triples(self, protein=0):
        return set((s % 16, te % 16, e - te) for o, te, e, s, _ in self.walk(protein)
                   if s is not None)

    def spans(self, protein=0):
        return [row[:3] for row in self.walk(protein)]


def assembly_case(specs, seed, protein=0):
    """Units (source phase, destination phase of the payload's first byte or
    None, payload length, more text, the payload's first bytes); a source phase
    of None is a unit without a record.  The text part's length brings the
    payload to its destination phase, under the X-trim rule of `protein`, and
    `more text` is added to it.  The records are numbered and laid out in pay in
    orders of their own; an empty payload that `begins` with X lies at an X."""
    rnd = random.Random(seed)
    recs = [k for k, p in enumerate(specs) if p[0] is not None]
    lens = [specs[k][2] for k in recs]
    start, used = place(lens, [specs[k][0] for k in recs], shuffled(range(len(recs)), rnd), 1)
    pay = noise(seed, used + 16, avoid=X)
    ids = shuffled(range(len(recs)), rnd)
    rspan = np.zeros(2 * len(recs), dtype=np.uint64)
    for j, k in enumerate(recs):
        head = specs[k][4]
        pay[start[j]:start[j] + len(head)] = np.frombuffer(head, dtype=np.uint8)
        rspan[2 * ids[j]] = start[j]
        rspan[2 * ids[j] + 1] = start[j] + lens[j]
        assert len(head) <= max(lens[j], 1)
    text = noise(seed + 1, 4096)
    units = np.zeros(len(specs), dtype=UNIT_DTYPE)
    at, cap, j = 0, 0, 0
    for k, (s, d, n, more, head) in enumerate(specs):
        tl = more + (0 if d is None else (d - at) % 16)
        units[k] = (rnd.randrange(len(text) - tl + 1), tl, NO_RECORD if s is None else ids[j])
        j += s is not None
        at += tl + n - (1 if protein and n and head[:1] == b'X' else 0)
        cap += tl + n
    return AssemblyCase(units, text, rspan, pay, pattern(cap + GUARD))


def with_text_only_units(specs, rnd, every=7):
    """every 7th unit of the result has no record, and a third of those no text"""
    out = []
    for p in specs:
        if len(out) % every == every - 1:
            more = rnd.choice([0, rnd.randint(1, 47), rnd.randint(1, 47)])
            out.append((None, None, 0, more, b''))
        out.append(p)
    return out


def assembly_every_class():
    """The 12,800 units with a payload of every class, the text of unit i
    16 (i mod 3) bytes longer than its phase asks for, and a unit without a
    record in every 7th place between them."""
    rnd = random.Random(3)
    specs = [(s, d, n, 16 * (i % 3), b'') for i, (s, d, n) in enumerate(shuffled(TRIPLES, rnd))]
    return assembly_case(with_text_only_units(specs, rnd), 3)


def assembly_shapes():
    rnd = random.Random(10)
    return {name: assembly_case([(rnd.randrange(16), None, n, rnd.randint(0, 20), b'')
                                 for n in lens], 100 + i)
            for i, (name, lens) in enumerate(sorted(shape_lens().items()))}


def assembly_byte_loops():
    """A group whose byte loop takes two rounds (more than 512 byte-stored
    bytes), then one that takes three (more than 1,024): text parts are stored
    byte by byte"""
    rnd = random.Random(11)
    two = [(rnd.randrange(16), None, rnd.randint(0, 8), rnd.randint(40, 55), b'')
           for _ in range(GROUP)]
    three = [(rnd.randrange(16), None, rnd.randint(0, 8), rnd.randint(70, 85), b'')
             for _ in range(GROUP)]
    return assembly_case(two + three, 11)


def assembly_chunk_loops():
    rnd = random.Random(12)
    return assembly_case([(s, d, n, rnd.randint(0, 10) if d is None else 16, b'')
                          for s, d, n in loop_specs(rnd)], 12)


XTRIM_LENS = (2, 3, 15, 16, 17, 18, 31, 32, 33, 34, 40, 49, 50)


def assembly_xtrim():
    """Laid out for protein = 1: a payload that begins with X at every source
    phase (of the X) and every destination phase (of the byte behind it); at
    every source phase the payload that is X and nothing else, an empty payload
    that lies at an X, a payload with X in second place only and one with two."""
    rnd = random.Random(13)
    specs = [(s, d, XTRIM_LENS[(s + 5 * d) % len(XTRIM_LENS)], 16 * ((s + d) % 2), b'X')
             for s in range(16) for d in range(16)]
    for s in range(16):
        specs.append((s, rnd.randrange(16), 0, 0, b'X'))
        specs.append((s, rnd.randrange(16), rnd.choice((2, 3, 17, 40)), 0, b'aX'))
        specs.append((s, rnd.randrange(16), rnd.choice((2, 3, 18, 35)), 0, b'XX'))
        specs.append((s, rnd.randrange(16), 1, 0, b'X'))
    return assembly_case(with_text_only_units(shuffled(specs, rnd), rnd), 13, protein=1)


# ---------------------------------------------------------------------------
# the line modes of the byte index
# ---------------------------------------------------------------------------

TEXT_BLOCK = 4096
TEXT_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193,
                3 * TEXT_BLOCK + 5)
CR_PLACES = (0, 14, 15, 16, 1022, 1023, 1024, 4094, 4095, 4096)  # and n - 2, n - 1
FILL = ord('x')
TAIL = np.frombuffer((b'\r\n\rx\n\n\r\r' * 5)[:40], dtype=np.uint8)  # behind a text: must not show


def lines_model(text, check_cr=True, reason=0):
    """(pos, n_lines, status) of a text: the line starts and the text's end;
    the lowest line << 8 | reason over the CRs that are neither before an LF
    nor the text's last byte, or NO_STRAY"""
    text = np.asarray(text, dtype=np.uint8)
    n = len(text)
    pos = [0] + (np.flatnonzero(text == LF) + 1).tolist()
    if n and text[-1] != LF:
        pos.append(n)
    status = NO_STRAY
    if check_cr:
        cr = np.flatnonzero(text == CR)
        cr = cr[cr != n - 1]
        stray = cr[text[cr + 1] != LF]
        if len(stray):
            status = int(np.count_nonzero(text[:stray[0]] == LF)) << 8 | reason
    return np.array(pos, dtype=np.uint64), len(pos) - 1, status


def cr_places(n):
    return sorted(set(p for p in CR_PLACES + (n - 2, n - 1) if 0 <= p < n))


def one_cr_cases():
    """[(label, buffer, index_len)]: for every length of at least 2, one CR at
    each place of cr_places(), with an LF and with another byte behind it
    (behind the text, for its last byte: there also with nothing), and LFs
    before it so that its line is not 0."""
    cases = []
    for n in TEXT_LENGTHS:
        if n < 2:
            continue
        for p in cr_places(n):
            for name, after in (('lf', LF), ('other', ord('y'))):
                text = np.full(n, FILL, dtype=np.uint8)
                text[3:max(p - 1, 0):97] = LF
                text[p] = CR
                tail = []
                if p + 1 < n:
                    text[p + 1] = after
                else:
                    tail = [after]
                label = 'n %d, CR at %d, %s behind it' % (n, p, name)
                cases.append((label, np.concatenate([text, np.array(tail, dtype=np.uint8)]), n))
                if p + 1 == n and name == 'lf':
                    cases.append(('n %d, CR at %d, nothing behind it' % (n, p), text, n))
    return cases


def several_cr_cases():
    """[(label, text)] with more than one CR"""
    cases = []
    n = 3 * TEXT_BLOCK + 5
    # one stray per lane, wave and block on ascending lines; without the first k of them
    places = (5, 3 * 16 + 2, 1024 + 7, 2048 + 15, TEXT_BLOCK + 100, 2 * TEXT_BLOCK + 9, n - 3)
    for k in range(len(places)):
        text = np.full(n, FILL, dtype=np.uint8)
        text[11::61] = LF
        text[n - 1] = CR  # the text's last byte: never stray
        for p in places[k:]:
            text[p] = CR
            assert text[p + 1] != LF
        cases.append(('strays at %s' % (places[k:],), text))
    for at in (0, 16 * 70, TEXT_BLOCK + 16 * 3):
        # two strays in one lane's 16 bytes, an LF between them
        text = np.full(2 * TEXT_BLOCK, FILL, dtype=np.uint8)
        text[7:at:50] = LF
        text[at + 1], text[at + 3], text[at + 5] = CR, LF, CR
        cases.append(('two strays in the lane at %d' % at, text))
        # the lane's first CR is before an LF, its second is not
        text = text.copy()
        text[at + 1:at + 7] = np.frombuffer(b'\r\n\n\rxx', dtype=np.uint8)
        cases.append(('CR LF LF CR in the lane at %d' % at, text))
    for at in (0, 13, 14, 15, 1021, 1022, 1023, TEXT_BLOCK - 3, TEXT_BLOCK - 2, TEXT_BLOCK - 1):
        text = np.full(TEXT_BLOCK + 40, FILL, dtype=np.uint8)
        text[2:max(at - 1, 0):33] = LF
        text[at:at + 3] = (CR, CR, LF)
        cases.append(('CR CR LF at %d' % at, text))
        cases.append(('CR CR LF at %d, no other CR' % at, text[:at + 3]))
    draw = np.random.RandomState(77).randint(0, 50, size=n)
    for k in range(3):
        # from the k-th LF on, so that the first stray's line is not 0
        text = np.full(n, FILL, dtype=np.uint8)
        text[draw == 0] = LF
        text[draw == 1] = CR
        head = text[:np.flatnonzero(text == LF)[2 * k]]  # a view
        head[head == CR] = FILL
        cases.append(('random CRs and LFs, none before LF %d' % (2 * k), text))
    return cases
