"""The case builders of tests/wavecopy_expect.py cover what they say they cover
(no device): every (source phase, destination phase, length) class in each of
the three enumerations, the rounds of the two loops, the X-trim phases and the
CR placements, read back from the tables the device tests send.  The models are
pinned on cases small enough to write out."""

import numpy as np

import wavecopy_expect as wx

ALL = set(wx.TRIPLES)


def u8(b):
    return np.frombuffer(b, dtype=np.uint8).copy()


def test_the_classes():
    assert len(ALL) == 16 * 16 * 50 == 12800
    # 0 to 3 whole chunks at every destination phase, and both sides of the threshold
    for d in range(16):
        chunks = set(wx.deal(d, d, d + n)[0] for n in wx.LENS)
        assert chunks == ({0, 1, 2, 3} if d in (0, 15) else {0, 1, 2})
        assert any(((d + 15) & ~15) + 16 == d + n for n in wx.LENS)
        # a whole chunk behind every head, before every tail length
        assert set((d + n) % 16 for n in wx.LENS if wx.deal(d, d, d + n)[0]) == set(range(16))
    assert wx.deal(0, 0, 48) == (3, 0) and wx.deal(1, 1, 50) == (2, 17)
    assert wx.deal(3, 3, 31) == (0, 28) and wx.deal(3, 3, 32) == (1, 13)
    assert wx.deal(0, 40, 100) == (3, 52)  # a text part is stored byte by byte
    assert wx.pattern(70000).std() > 50 and len(set(wx.pattern(4096)[::256].tolist())) > 8


def test_models_on_small_cases():
    base = u8(b'0123456789abcdef')
    case = wx.PieceCase(base, [10, 0, 3], [1, 9, 5], [3, 0, 2], u8(b'................'))
    assert case.model().tobytes() == b'.abc.34.........'
    assert case.triples() == {(10, 1, 3), (0, 9, 0), (3, 5, 2)}
    seg = wx.SegmentCase(base, [10, 0, 3], [2, 5, 5, 7], u8(b'..........'))
    assert seg.model().tobytes() == b'..abc34...'
    assert seg.triples() == {(10, 2, 3), (0, 5, 0), (3, 5, 2)}
    units = np.array([(0, 2, 1), (2, 0, wx.NO_RECORD), (1, 3, 0), (0, 0, 2), (4, 1, 3)],
                     dtype=wx.UNIT_DTYPE)
    asm = wx.AssemblyCase(units, u8(b'>id\n-'), [0, 3, 3, 7, 7, 8, 8, 8], u8(b'XACGTTAXX'),
                          u8(b'....................'))
    want0, n0 = asm.model(0)
    want1, n1 = asm.model(1)
    assert want0[:n0].tobytes() == b'>iGTTAid\nXACX-' and (want0[n0:] == ord('.')).all()
    assert want1[:n1].tobytes() == b'>iGTTAid\nAC-' and (want1[n1:] == ord('.')).all()
    # the empty record 3 lies at an X: nothing is trimmed from nothing
    assert [row[4] for row in asm.walk(1)] == [False, False, True, True, False]
    assert asm.triples(1) == {(3, 2, 4), (1, 9, 2), (8, 11, 0), (8, 12, 0)}
    for text, pos, stray in ((b'', [0], None), (b'\n', [0, 1], None), (b'ab\ncd', [0, 3, 5], None),
                             (b'ab\r\ncd\r', [0, 4, 7], None), (b'a\n\n\rb\n', [0, 2, 3, 6], 2),
                             (b'\r\r\n', [0, 3], 0), (b'a\nb\r', [0, 2, 4], None),
                             (b'a\nb\rc\n\rd', [0, 2, 6, 8], 1)):
        got, n_lines, status = wx.lines_model(u8(text), True, 0x5a)
        assert got.tolist() == pos and n_lines == len(pos) - 1, text
        assert status == (wx.NO_STRAY if stray is None else stray << 8 | 0x5a), text
        assert wx.lines_model(u8(text), False, 0x5a)[2] == wx.NO_STRAY


def test_piece_copy_enumerates_every_class():
    case = wx.piece_every_class()
    assert len(case.src) == 12800 and case.triples() == ALL
    assert len(case.out) < 1 << 20
    order = np.argsort(case.dst, kind='stable')
    start, end = case.dst[order], case.dst[order] + case.len[order]
    assert start[0] >= 1 and (end[:-1] < start[1:]).all()  # an untouched byte between neighbours
    assert int(end[-1]) + wx.GUARD <= len(case.out)
    assert (case.src + case.len <= len(case.base)).all()
    for k in range(0, 12800, wx.GROUP):  # a group mixes the classes
        assert len(set(case.len[k:k + wx.GROUP].tolist())) >= 6
        assert len(set((case.dst[k:k + wx.GROUP] % 16).tolist())) >= 4
    assert not np.array_equal(case.model(), case.out)


def test_segments_enumerate_every_class():
    case = wx.segment_every_class()
    assert case.triples() >= ALL
    n = len(case.src_off)
    assert 24000 < n < 25600 and len(case.dst_off) == n + 1  # the fillers are segments
    assert case.dst_off[0] == wx.SEGMENT_START == 5
    assert len(case.dst) == int(case.dst_off[-1]) + wx.GUARD < 1 << 20
    assert (case.src_off + np.diff(case.dst_off) <= len(case.src)).all()


def test_assembly_enumerates_every_class():
    case = wx.assembly_every_class()
    assert case.triples(0) >= ALL
    rec = case.units['rec']
    assert np.count_nonzero(rec != wx.NO_RECORD) == 12800
    seventh = np.arange(len(rec)) % 7 == 6
    assert (rec[seventh] == wx.NO_RECORD).all() and (rec[~seventh] != wx.NO_RECORD).all()
    assert sorted(rec[rec != wx.NO_RECORD].tolist()) == list(range(12800))
    assert set(case.units['text_len'].tolist()) == set(range(48))
    rows = case.walk(0)
    assert sum(1 for o, te, e, s, _ in rows if o == e and s is not None) >= 3  # both parts empty
    assert sum(1 for o, te, e, s, _ in rows if o == e and s is None) >= 3
    want, n = case.model(0)
    assert n == rows[-1][2] == len(case.out) - wx.GUARD < 1 << 20
    assert np.array_equal(want[n:], case.out[n:])


def test_group_shapes():
    lens = wx.shape_lens()
    for n in wx.GROUP_SIZES:
        assert len(lens['n%d' % n]) == n
    assert lens['zero_group'][16:32] == [0] * 16 and all(lens['zero_group'][:16])
    edges = lens['zero_edges']
    groups = [edges[k:k + 16] for k in range(0, len(edges), 16)]
    assert [len(g) for g in groups] == [16, 16, 16, 4]
    assert groups[0][0] == groups[0][-1] == 0 and all(groups[0][1:-1])
    assert groups[1][:2] == groups[1][-2:] == [0, 0] and groups[2][-1] == 0 and groups[3][0] == 0
    pieces, segments, units = wx.piece_shapes(), wx.segment_shapes(), wx.assembly_shapes()
    assert len(pieces.pop('n0').src) == 0
    assert set(pieces) == set(segments) == set(units) == set(lens)
    for name, want in lens.items():
        assert pieces[name].len.tolist() == want
        assert np.diff(segments[name].dst_off).tolist() == want
        assert [e - te for o, te, e, s, _ in units[name].walk(0)] == want
        assert not np.array_equal(pieces[name].model(), pieces[name].out)


def test_loop_rounds():
    for k, s, d, n in wx.LONG_PIECES:
        assert s % 2 and d % 2 and s != d
    # the tiny pieces alone stay in the first round; 4,200 bytes reach the second, 8,400 the third
    assert [r[0] for r in wx.rounds(wx.piece_loops().spans())][1:] == [2, 3]
    assert (4200, 8400) == tuple(n for k, s, d, n in wx.LONG_PIECES)
    assert {(3, 9, 4200), (13, 7, 8400)} <= wx.piece_loops().triples()
    seg = wx.segment_loops()
    assert {2, 3} <= set(r[0] for r in wx.rounds(seg.spans()))
    assert (3, 9, 4200) in seg.triples() and (13, 7, 8400) in seg.triples()
    asm = wx.assembly_chunk_loops()
    assert [r[0] for r in wx.rounds(asm.spans())][1:] == [2, 3]
    assert (3, 9, 4200) in asm.triples() and (13, 7, 8400) in asm.triples()
    # the piece copy cannot reach the byte loop's second round
    most = max(wx.deal(d, d, d + n)[1] for d in range(16) for n in range(200))
    assert most == 30 and wx.GROUP * most < wx.BYTE_ROUND
    assert [r[1] for r in wx.rounds(wx.assembly_byte_loops().spans())] == [2, 3]


def test_xtrim_phases():
    case = wx.assembly_xtrim()
    span, pay = case.rspan.tolist(), case.pay
    rows1, rows0 = case.walk(1), case.walk(0)
    assert not any(row[4] for row in rows0)
    trimmed = [row for row in rows1 if row[4]]
    # the X's source phase (the payload then starts one byte on) x the destination phase
    assert set(((s - 1) % 16, te % 16) for o, te, e, s, _ in trimmed if e > te) == \
        set((s, d) for s in range(16) for d in range(16))
    assert set((s - 1) % 16 for o, te, e, s, _ in trimmed if e == te) == set(range(16))  # 'X' alone
    first = lambda r: pay[span[2 * r]]
    recs = range(len(span) // 2)
    empty_at_x = [r for r in recs if span[2 * r] == span[2 * r + 1] and first(r) == wx.X]
    second = [r for r in recs if span[2 * r + 1] - span[2 * r] >= 2 and first(r) != wx.X and
              pay[span[2 * r] + 1] == wx.X]
    double = [r for r in recs if span[2 * r + 1] - span[2 * r] >= 2 and first(r) == wx.X and
              pay[span[2 * r] + 1] == wx.X]
    assert len(empty_at_x) == len(second) == len(double) == 16
    assert set(span[2 * r] % 16 for r in empty_at_x) == set(range(16))
    assert len(trimmed) == sum(1 for r in recs
                               if span[2 * r + 1] > span[2 * r] and first(r) == wx.X)
    n0, n1 = case.model(0)[1], case.model(1)[1]
    assert n0 - n1 == len(trimmed) and n0 + wx.GUARD == len(case.out)
    assert (case.units['rec'] == wx.NO_RECORD).any()


def test_cr_placements():
    cases = wx.one_cr_cases()
    seen = {}
    for label, buf, n in cases:
        at = np.flatnonzero(buf[:n] == wx.CR)
        assert len(at) == 1 and not (buf[n:] == wx.CR).any(), label
        p = int(at[0])
        after = int(buf[p + 1]) if p + 1 < len(buf) else None
        seen.setdefault((n, p), set()).add('none' if after is None else 'lf' if after == wx.LF
                                           else 'other')
        pos, n_lines, status = wx.lines_model(buf[:n], True, 2)
        if p == n - 1 or after == wx.LF:
            assert status == wx.NO_STRAY, label
        else:
            assert status & 255 == 2 and (status >> 8 > 0) == (p >= 5), label
            assert status >> 8 == np.count_nonzero(buf[:p] == wx.LF), label
        assert pos[n_lines] == n
    want = {}
    for n in wx.TEXT_LENGTHS:
        for p in set(wx.CR_PLACES + (n - 2, n - 1)):
            if n >= 2 and 0 <= p < n:
                want[(n, p)] = {'lf', 'other', 'none'} if p == n - 1 else {'lf', 'other'}
    assert seen == want and len(want) > 100
    several = wx.several_cr_cases()
    lines = []
    for label, text in several:
        status = wx.lines_model(text, True, 0)[2]
        assert np.count_nonzero(text == wx.CR) >= 2 and status != wx.NO_STRAY, label
        lines.append(status >> 8)
    assert lines[:7] == sorted(set(lines[:7])) and lines[0] == 0  # each one in turn is the lowest
    assert sum(1 for label, _ in several if label.startswith('random')) == 3
    assert (wx.TAIL == wx.LF).any() and (wx.TAIL == wx.CR).any() and len(wx.TAIL) == 40
