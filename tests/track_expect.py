"""What position_dic must give (genome.py:981-1100), restated in numpy, and
the loader of the reference's own recorded results
(tests/golden/position_dic.json, written by golden/make_golden_positions.py).
Not a test module: test_position_dic.py and test_gpu_track.py import it, and
so does the golden generator, for the one encoding of results both sides use."""

import hashlib
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden')
LONG = 300  # lists above this many entries are stored as sha256 + length
OBIROI_FA = 'O.biroi_refseqGenomeSubset.fasta'
OBIROI_GFF = 'O.biroi_NCBIrefseq_gff3Subset.gff'


# -- encoding ---------------------------------------------------------------

def plain(x):
    """numpy scalars, tuples and sets as the JSON-able Python values."""
    if isinstance(x, (np.bool_, bool)):
        return bool(x)
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    if isinstance(x, (set, frozenset)):
        return sorted(plain(v) for v in x)
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    return x


def digest(obj):
    return hashlib.sha256(json.dumps(obj, separators=(',', ':')).encode()).hexdigest()


def encode_list(lst):
    lst = plain(list(lst))
    if len(lst) > LONG:
        return {'sha': digest(lst), 'n': len(lst)}
    return lst


def encode_array(arr):
    arr = np.asarray(arr)
    if arr.dtype == np.bool_:
        raw = np.packbits(arr, bitorder='little').tobytes()
        if len(arr) > 4096:
            return {'bits_sha': hashlib.sha256(raw).hexdigest(), 'n': len(arr),
                    'ones': int(np.count_nonzero(arr))}
        return {'bits': raw.hex(), 'n': len(arr)}
    return {'values': encode_list(arr.tolist())}


def decode_bits(enc):
    raw = np.frombuffer(bytes.fromhex(enc['bits']), np.uint8)
    return np.unpackbits(raw, bitorder='little')[:enc['n']].astype(bool)


def encode_arrays(pd):
    return {seqid: encode_array(pd[seqid]) for seqid in pd}


def encode_result(res):
    """A method's return value: a dict of lists, an annotation set with a
    ``region`` dict, a list, or None."""
    if res is None:
        return None
    if hasattr(res, 'region'):
        return {'regions': encode_list([[r.ID, r.seqid, list(r.coords), r.feature_type]
                                        for r in res.region.values()])}
    if isinstance(res, dict):
        return {'dict': {k: encode_list(v) for k, v in res.items()}, 'keys': list(res)}
    return {'list': encode_list(res)}


def sha_text(text):
    return hashlib.sha256(text.encode('latin-1')).hexdigest()


def load():
    with open(os.path.join(GOLDEN, 'position_dic.json')) as fh:
        return json.load(fh)


# -- restatements -----------------------------------------------------------

def base_class(seq, gc=False):
    """bool per byte: in ATat (or CGcg)."""
    b = np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else np.asarray(seq)
    letters = b'CGcg' if gc else b'ATat'
    out = np.zeros(len(b), bool)
    for ch in letters:
        out |= b == ch
    return out


def n_windows(length, window, jump):
    return (length - window) // jump if length > window else 0


def window_sums(arr, window, jump):
    """Sum of arr[i * jump:i * jump + window] for i < (len - window) // jump."""
    n = n_windows(len(arr), window, jump)
    c = np.concatenate([[0], np.cumsum(np.asarray(arr, dtype=np.int64))])
    starts = np.arange(n, dtype=np.int64) * jump
    return c[starts + window] - c[starts]


def regions_walk(passes, window, jump, length):
    """genome.py:1061-1085 over every window: ``passes[i]`` is the threshold
    test of window i.  The coords lists of one contig."""
    coords_list = []
    window_in = False
    for position, ok in enumerate(passes):
        window_start = position * jump
        if ok:
            if not window_in:
                window_in = True
                if len(coords_list) == 0:
                    coords_list.append([1 + window_start])
                elif position > coords_list[-1][1]:
                    coords_list.append([1 + window_start])
        elif window_in:
            window_in = False
            if len(coords_list[-1]) == 1:
                coords_list[-1].append(window_start + window)
            else:
                coords_list[-1][1] = window_start + window
    if coords_list and len(coords_list[-1]) == 1:
        coords_list[-1].append(length)
    return coords_list


def regions_from_flips(flips, window, jump, length):
    """The same walk over the flip positions only (what the device returns)."""
    passes_at = {}
    state = False
    for p in flips:
        state = not state
        passes_at[int(p)] = state
    coords_list = []
    window_in = False
    for position in sorted(passes_at):
        window_start = position * jump
        if passes_at[position]:
            window_in = True
            if len(coords_list) == 0 or position > coords_list[-1][1]:
                coords_list.append([1 + window_start])
        else:
            window_in = False
            if len(coords_list[-1]) == 1:
                coords_list[-1].append(window_start + window)
            else:
                coords_list[-1][1] = window_start + window
    if coords_list and len(coords_list[-1]) == 1:
        coords_list[-1].append(length)
    return coords_list


def flips_of(passes):
    passes = np.asarray(passes, dtype=bool)
    before = np.concatenate([[False], passes])[:-1]
    return np.flatnonzero(passes != before)


def counts(arr, first, stop):
    """[zeros, ones] of arr[first:stop] (inside the array)."""
    part = np.asarray(arr[first:stop])
    return [int(np.count_nonzero(part == 0)), int(np.count_nonzero(part == 1))]


def at_content_lines(data):
    """genome_tools.py:506-524 on a file's bytes (lines end at '\\n'): the
    printed text."""
    out = []
    name = ats = gcs = None
    for line in data.split(b'\n'):
        line += b'\n'
        if line == b'\n':
            continue
        if b'>' in line:
            if name is not None:
                out.append(name + b'%d\t%d\n' % (ats, gcs))
            name = line[1:].replace(b'\n', b'').replace(b'\r', b'') + b'\t'
            ats = gcs = 0
        else:
            up = line.upper()
            ats += up.count(b'A') + up.count(b'T')
            gcs += up.count(b'G') + up.count(b'C')
    out.append(name + b'%d\t%d\n' % (ats, gcs))
    return b''.join(out)


# -- the case runner (the reference in the generator, magot_amd in the tests) --

def capture(fn):
    """(result, exception name, captured stdout)."""
    import contextlib
    import io
    buf = io.StringIO()
    res = exc = None
    with contextlib.redirect_stdout(buf):
        try:
            res = fn()
        except Exception as e:  # noqa: BLE001
            exc = type(e).__name__
    return res, exc, buf.getvalue()


def genome_of(mod, genomes, name, cache):
    key = (mod.__name__, name)
    if key not in cache:
        if name == 'obiroi':
            cache[key] = mod.GenomeSequence(os.path.join(GOLDEN, OBIROI_FA))
        else:
            g = mod.GenomeSequence()
            for seqid, seq in genomes[name]:
                g[seqid] = seq
            cache[key] = g
    return cache[key]


def annotations_of(mod, spec, cache):
    if 'gff_file' in spec:
        key = (mod.__name__, spec['gff_file'])
        if key not in cache:
            cache[key] = mod.read_gff(os.path.join(GOLDEN, spec['gff_file']))
        return cache[key]
    aset = mod.AnnotationSet()
    table = {}
    for ID, seqid, first, last in spec['features']:
        table[ID] = mod.BaseAnnotation(ID, seqid, (first, last), spec['feature'],
                                       annotation_set=aset)
    setattr(aset, spec['feature'], table)
    return aset


def apply_step(mod, pd, step, genomes, cache, kw, jump_wrap=int):
    op = step['op']
    if op == 'at_content':
        return pd.at_content(genome_of(mod, genomes, step['genome'], cache), **kw)
    if op == 'fill':
        return pd.fill_from_annotations(annotations_of(mod, step['ann'], cache),
                                        step['ann']['feature'], fill_type=step['fill_type'],
                                        fill_with=step['fill_with'], **kw)
    if op == 'count':
        return pd.count_from_annotations(annotations_of(mod, step['ann'], cache),
                                         step['ann']['feature'], **kw)
    if op == 'sliding':
        a = dict(step['kw'])
        a['window_jump'] = jump_wrap(a.get('window_jump', 1))
        return pd.sliding_window_calculate(**a, **kw)
    raise ValueError(op)


def run_case(mod, case, genomes, cache, native=None, jump_wrap=int):
    """(position_dic, result, exception name, stdout) of one recorded case."""
    kw = {} if native is None else {'native': native}
    g = genome_of(mod, genomes, case['genome'], cache)
    pd = mod.position_dic(g, dtype=bool if case['dtype'] == 'bool' else int)
    was = mod.verbose
    mod.verbose = False
    try:
        for step in case['setup']:
            apply_step(mod, pd, step, genomes, cache, kw, jump_wrap)
        mod.verbose = bool(case['call'].get('verbose'))
        res, exc, out = capture(lambda: apply_step(mod, pd, case['call'], genomes, cache, kw,
                                                   jump_wrap))
    finally:
        mod.verbose = was
    return pd, res, exc, out


def outcome(pd, res, exc, out):
    """What a case records of a run."""
    text = {'stdout': out} if len(out) <= 4096 else {'stdout_sha': sha_text(out), 'stdout_n': len(out)}
    return dict(text, exc=exc, result=encode_result(res), arrays=encode_arrays(pd))
