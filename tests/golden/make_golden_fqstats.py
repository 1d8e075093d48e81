"""Record what the REFERENCE's own fqstats prints: tests/golden/fqstats.json.

Runs only where the reference is installed (see make_golden.py, whose
lib2to3 copy this imports); the reference function (genome_tools.py:85-124)
runs unchanged, and nothing of its program text is stored: only inputs,
outputs and exception names.

The copy runs under Python 3, which differs from the Python 2 target in two
places this function touches; both are handled here, in the namespace the
copy's function looks its names up in, not in the copy:

  * ``open``: text mode would translate line ends and decode UTF-8.  The
    shadow opens with ``newline='\\n'`` (lines end at LF only, nothing is
    translated) and ``encoding='latin-1'`` (one character per byte).
  * ``/`` on integers is a true division.  ``len`` and ``sum`` are shadowed
    by versions that return an ``int`` subclass whose ``/`` floors and whose
    arithmetic returns the subclass again, so every figure the function
    derives from them divides as Python 2 does, zero included.

Per case: ``text`` (the file's bytes as latin-1), ``out`` (stdout) and ``exc``
(exception name, or null).

Usage:  python tests/golden/make_golden_fqstats.py
"""

import builtins
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
import fqstats_expect as fe  # noqa: E402


class Py2Int(int):
    """An int whose ``/`` floors, closed under its arithmetic"""

    def __truediv__(self, other):
        return Py2Int(int(self) // int(other))

    def __rtruediv__(self, other):
        return Py2Int(int(other) // int(self))


def _closed(name):
    plain = getattr(int, name)

    def method(self, other):
        res = plain(int(self), int(other))
        return res if res is NotImplemented else Py2Int(res)
    method.__name__ = name
    return method


for _name in ('__add__', '__radd__', '__sub__', '__rsub__', '__mul__', '__rmul__',
              '__floordiv__', '__rfloordiv__', '__mod__', '__rmod__'):
    setattr(Py2Int, _name, _closed(_name))


def shadow(tools):
    tools.open = lambda path, *a, **k: builtins.open(path, newline='\n', encoding='latin-1')
    tools.len = lambda x: Py2Int(builtins.len(x))
    tools.sum = lambda x: Py2Int(builtins.sum(x))


def cases():
    """name -> bytes"""
    rec = fe.record
    c = {}
    c['example'] = b''.join(rec(b'r%d' % k, n) for k, n in
                            enumerate([5, 12, 7, 30, 30, 2, 19, 100, 45, 8, 61]))
    c['one_read'] = rec(b'r', 9)
    c['two_reads'] = rec(b'a', 4) + rec(b'b', 11)
    c['crlf'] = b''.join(rec(b'r%d' % k, n, eol=b'\r\n') for k, n in enumerate([5, 12, 7, 30, 0]))
    c['no_final_lf_sequence'] = rec(b'a', 6) + b'@b\nACGTACGT'
    c['no_final_lf_sequence_one_byte'] = rec(b'a', 6) + b'@b\nA'
    c['no_final_lf_quality'] = (rec(b'a', 6) + rec(b'b', 3))[:-1]
    c['no_final_lf_header'] = rec(b'a', 6) + b'@b'
    c['no_final_lf_crlf'] = b''.join(rec(b'r%d' % k, n, eol=b'\r\n') for k, n in
                                     enumerate([3, 8]))[:-1]
    for extra in range(4):  # line counts = 0, 1, 2, 3 (mod 4)
        c['lines_mod4_%d' % extra] = rec(b'a', 10) + rec(b'b', 20) + \
            b''.join([b'@c\n', b'ACGTACG\n', b'+\n'][:extra])
    c['empty_sequences_only'] = rec(b'a', 0) + rec(b'b', 0) + rec(b'c', 0)
    c['one_empty_sequence'] = rec(b'a', 0)
    c['one_base'] = rec(b'a', 0) + rec(b'b', 1) + rec(b'c', 0)
    c['one_base_alone'] = rec(b'a', 1)
    c['two_bases'] = rec(b'a', 1) + rec(b'b', 1)
    c['empty_file'] = b''
    c['one_line'] = b'@a\n'
    c['one_line_no_lf'] = b'@a'
    c['one_lf'] = b'\n'
    c['lone_cr_in_sequence'] = b'@a\nACGT\rACGT\n+\nIIII\rIIII\n' + rec(b'b', 5)
    c['lone_cr_in_header'] = b'@a\rACGTACGTACGT\nAC\n+\nII\n' + rec(b'b', 7)
    c['only_lfs'] = b'\n' * 11
    c['content_is_not_checked'] = b'ACGT\n@name\nIIII\n+\n' * 3
    c['equal_lengths'] = b''.join(rec(b'r%d' % k, 150) for k in range(9))
    c['high_bytes'] = b'@\xe9\n\xff\xfe\x80AC\n+\n\x00\x01III\n'
    rng = np.random.default_rng(20261019)
    for k in range(8):
        c['random_%02d' % k] = fe.random_fastq(rng, eol=b'\r\n' if k % 6 == 5 else b'\n')
    return c


def main():
    make_golden.reference_module()
    import genome_tools as tools
    shadow(tools)
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'reads.fastq')
        for name, data in cases().items():
            with open(path, 'wb') as fh:
                fh.write(data)
            _, exc, text = make_golden.call(lambda: tools.fqstats(path))
            out[name] = {'text': data.decode('latin-1'), 'out': text, 'exc': exc}
            print(name, exc, text.split('\n')[0], flush=True)
        _, exc, text = make_golden.call(lambda: tools.fqstats(os.path.join(tmp, 'absent.fastq')))
        assert (exc, text) == ('FileNotFoundError', ''), (exc, text)
    with open(os.path.join(HERE, 'fqstats.json'), 'w') as fh:
        json.dump({'cases': out}, fh, indent=0, sort_keys=True)
        fh.write('\n')


if __name__ == '__main__':
    main()
