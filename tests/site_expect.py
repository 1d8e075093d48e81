"""What composition_by_site must print (genome_tools.py:488-503), written from
the reference's semantics and used as the expectation of the host tests, the
GPU tests and the golden generator's case table.

The records are GenomeSequence's: a line that starts with '>' names the next
record (CR and LF removed), every other line adds its bytes without CR and LF
to the record open; text before the first header is the record named '';
an empty record is dropped; a repeated name keeps its first position and
takes the last sequence.  The number of sites is the length of the dict's
first record -- first in the file, or first in the order a Python 2 dict of
the names iterates.  Per site, the records holding a, t, c or g in either
case are counted; the line is the four shares of their sum as Python 2's
str(float) prints them.  A record that ends before a site raises IndexError
there, a site without a counted base ZeroDivisionError there, whichever site
comes first; no record at all raises IndexError.  Nothing is printed then.
"""

import json
import os

import numpy as np

from oracle import magot_oracle as mo

HERE = os.path.dirname(os.path.abspath(__file__))
ORDERS = ('insertion', 'py2')
COLUMNS = b'atcg'
TALL_ROWS = 30000


def load():
    with open(os.path.join(HERE, 'golden', 'site.json')) as fh:
        return json.load(fh)


def py2_float_str(value):
    """Python 2's str(float): '%.12g', '.0' added to what has no '.' or 'e'"""
    text = '%.12g' % value
    return text if ('.' in text or 'e' in text) else text + '.0'


def records(text):
    """The dict GenomeSequence builds of the bytes ``text``, in insertion order"""
    out = {}
    name, seq = b'', b''
    for line in text.split(b'\n'):
        if line[:1] == b'>':
            if seq:
                out[name] = seq
                seq = b''
            name = line[1:].replace(b'\r', b'')
        else:
            seq += line.replace(b'\r', b'')
    if seq:
        out[name] = seq
    return out


def first_name(names, order):
    if order == 'py2':
        return mo.py2_dict_order([n.decode('latin-1') for n in names])[0].encode('latin-1')
    return names[0]


def counts_of(rows, n_sites):
    """n_sites x 4 counts (a, t, c, g) of rows at least n_sites long: a list of
    bytes, or a 2-D uint8 array"""
    if isinstance(rows, np.ndarray):
        cells = rows[:, :n_sites]
    else:
        cells = np.array([np.frombuffer(r[:n_sites], np.uint8) for r in rows], np.uint8)
        cells = cells.reshape(len(rows), n_sites)
    cells = np.where((cells >= ord('A')) & (cells <= ord('Z')), cells | 0x20, cells)
    out = np.zeros((n_sites, 4), np.uint32)
    for k, base in enumerate(COLUMNS):
        out[:, k] = (cells == base).sum(axis=0)
    return out


def render(counts):
    lines = ['a\tt\tc\tg\n']
    for row in np.asarray(counts).tolist():
        total = sum(row)
        lines.append('\t'.join(py2_float_str(c * 1.0 / total) for c in row) + '\n')
    return ''.join(lines)


def expected(text, order):
    """(stdout as str, exception name or None) of the tool on the bytes ``text``"""
    recs = records(text)
    if not recs:
        return '', 'IndexError'
    names = list(recs)
    n_sites = len(recs[first_name(names, order)])
    shortest = min(len(r) for r in recs.values())
    counts = counts_of(list(recs.values()), min(n_sites, shortest))
    if not counts.any(axis=1).all():
        return '', 'ZeroDivisionError'
    if shortest < n_sites:
        return '', 'IndexError'
    return render(counts), None


def tall_text():
    """TALL_ROWS records of one base, a single 'A' among 'T's: 1 / 30000 is
    printed in the exponent form"""
    return b''.join(b'>%x\n%s\n' % (k, b'A' if k == 7 else b't') for k in range(TALL_ROWS))


def text_of(case):
    """The input bytes of a recorded case"""
    if case['text'] is None:
        assert case['gen'] == 'tall'
        return tall_text()
    return case['text'].encode('latin-1')


def note_of(note, order):
    return note[order] if isinstance(note, dict) else note


def cases():
    """name -> (text, note).  The note is 'native' where the device path must
    answer; the exception it must raise itself ('IndexError',
    'ZeroDivisionError'); or the reason it must decline to the host loop.  A
    dict where the two orders differ."""
    thirds = b'>p\nAAAAAA\n>q\nATTCCG\n>r\nTTCGGN\n'
    return {
        'plain': (b'>s1\nACGTAC\n>s2\nACGTTC\n>s3\nTCGTAC\n>s4\nACGAAC\n', 'native'),
        'wrapped': (b'>s1\nACG\nTACGT\nA\n>s2\nACGTACGTA\n>s3\nAC\nGT\nAC\nGT\nT\n', 'native'),
        'crlf': (b'>s1 one\r\nACGT\r\nAC\r\n>s2\r\nAGGTTC\r\n', 'native'),
        'no_final_newline': (b'>s1\nACGT\n>s2\nAGGT', 'native'),
        'lower_mixed': (b'>s1\nacgtAC\n>s2\nAcGtac\n>s3\ntTgGaA\n', 'native'),
        'uncounted': (b'>s1\nAN-RAC T\n>s2\nCnYy-C*A\n>s3\nGAtgGGcW\n', 'native'),
        'longer_later': (b'>s1\nACGT\n>s2\nACGTGGGG\n>s3\nTTTTAAAACCCC\n', {'insertion': 'native',
                                                                        'py2': 'IndexError'}),
        'shorter_later': (b'>y\nACGTAC\n>x\nACG\n>z\nACGTAC\n', 'IndexError'),
        'shorter_first_in_one_order': (b'>s1\nACG\n>s2\nACGT\n>s3\nACGTA\n',
                                       {'insertion': 'native', 'py2': 'IndexError'}),
        'empty_column': (b'>s1\nAC-T\n>s2\nACNT\n', 'ZeroDivisionError'),
        'empty_column_before_short_row': (b'>y\nA-GTAC\n>x\nAN\n>z\nA-GTAC\n', 'ZeroDivisionError'),
        'empty_column_after_short_row': (b'>y\nACG-AC\n>x\nAC\n>z\nACGNAC\n', 'IndexError'),
        # the native reader folds it as the dict does: first position, last sequence
        'repeated_name': (b'>a\nACGT\n>a\nTT\n>b\nACGT\n', 'native'),
        'repeated_name_shortens': (b'>s1\nACG\n>s3\nACGTA\n>s3\nAC\n',
                                   {'insertion': 'IndexError', 'py2': 'native'}),
        'text_before_header': (b'AC\n>s1\nAG\n>s2\nAT\n', 'text before the first header'),
        'empty_file': (b'', 'no records'),
        'headers_only': (b'>s1\n>s2\n', 'no records'),
        'empty_record': (b'>s1\n>s2\nACGT\n>s3\n\n>s4\nAGGT\n', 'native'),
        'one_row': (b'>only\nACGTNacgt-\n', 'ZeroDivisionError'),
        'one_row_counted': (b'>only\nACGTacgt\n', 'native'),
        'thirds': (thirds, 'native'),
        'sevenths': (b''.join(b'>r%d\n%s\n' % (k, (b'A' * k + b'C' * (7 - k)) + b'ACGTACG'[k:] +
                                               b'ACGTACG'[:k]) for k in range(7)), 'native'),
        'protein': (b'>p1\nMKTAYIAKQR\n>p2\nMKTGYLAKCR\n', 'ZeroDivisionError'),
        'protein_counted': (b'>p1\nATGC\n>p2\nTAGC\n>p3\nCCGA\n', 'native'),
        'tall': (None, 'native'),
    }
