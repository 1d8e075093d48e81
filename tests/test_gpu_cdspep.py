"""genome_tools.get_CDS_peptides on the device and on the object path against
the reference's recorded output (tests/golden/get_cds_peptides.json, insertion
order) and the closed form of tests/cdspep_expect.py (both orders): byte for
byte, with exception names, the path taken and the partial file."""

import json
import os

import pytest

import cdspep_expect as ce
import orfs_expect as oe
from magot_amd import genome_tools

pytestmark = pytest.mark.gpu

# (path the tool takes with native=True, why it takes the object path)
PATHS = {'obiroi': ('host', 'the annotation takes a diagnostic path'),
         'names_invalid': ('host', 'invalid names_from'),
         'no_annotations': ('host', 'read_gff takes a diagnostic path')}


@pytest.fixture(scope='module')
def golden(golden_dir):
    with open(os.path.join(golden_dir, 'get_cds_peptides.json')) as fh:
        return json.load(fh)['cases']


@pytest.fixture(scope='module')
def inputs(golden_dir, tmp_path_factory):
    """name -> (fasta path, gff path, keywords, fasta text, gff text), written once."""
    out = {}
    for name in ce.TOOL_CASES:
        d = tmp_path_factory.mktemp(name)
        fasta, gff, kw = ce.tool_inputs(name, golden_dir)
        (d / 'in.fa').write_bytes(fasta.encode('latin-1'))
        (d / 'in.gff').write_bytes(gff.encode('latin-1'))
        out[name] = (str(d / 'in.fa'), str(d / 'in.gff'), kw, fasta, gff)
    return out


def run(fa, gff, out, kw, capsys=None, **more):
    if os.path.exists(out):
        os.remove(out)
    exc = None
    try:
        genome_tools.get_CDS_peptides(fa, gff, out, **dict(kw, **more))
    except (IndexError, KeyError, AttributeError) as e:
        exc = type(e).__name__
    if not os.path.exists(out):
        return None, exc  # raised before the output file was opened
    with open(out, 'rb') as fh:
        return fh.read().decode('latin-1'), exc


@pytest.mark.parametrize('name', sorted(ce.TOOL_CASES))
def test_tool_against_the_reference(name, golden, inputs, tmp_path, capsys):
    fa, gff, kw, fasta_text, gff_text = inputs[name]
    want = golden[name]
    out = str(tmp_path / 'out.fa')
    path, why = PATHS.get(name, ('native', None))
    # the device path, then the object path (c14: the GTF, 2596 CDS in one batch)
    for native, last in (('True', (path, why)), ('False', ('host', "native != 'True'"))):
        got, exc = run(fa, gff, out, kw, order='insertion', native=native)
        assert (got is not None) == want['file']
        got = got or ''
        assert (oe.sha(got), len(got), exc) == (want['sha'], want['size'], want['exc'])
        if 'out' in want:
            assert got == want['out']
        assert capsys.readouterr().out == want['stdout']
        assert genome_tools.get_CDS_peptides.last_path == ('get_CDS_peptides',) + last
    # Python 2 dict order, the default: the closed form
    want_text, want_exc = ce.tool_text(fasta_text, gff_text, order='py2', **kw)
    got, exc = run(fa, gff, out, kw)
    assert (got, exc) == (want_text, want_exc)


def test_partial_file_when_a_cds_has_no_orf(golden, inputs, tmp_path):
    """The NNN CDS is the second of three in its transcript: the reference
    computes the transcript's ORFs before it writes one, so the file ends with
    the transcript before it, on both paths."""
    fa, gff, kw, _, _ = inputs['nnn_middle']
    out = str(tmp_path / 'out.fa')
    for native in ('True', 'False'):
        got, exc = run(fa, gff, out, kw, order='insertion', native=native)
        assert exc == 'IndexError' and got == golden['nnn_middle']['out']
        assert got.split('>')[-1].startswith('c3.1a\n') and 'c3.2a' not in got
    assert golden['basic']['out'].startswith(got) and 'c3.2a' in golden['basic']['out']


def test_command_line(golden, inputs, tmp_path):
    fa, gff, _, _, _ = inputs['basic']
    out = str(tmp_path / 'cli.fa')
    argv = ['get_CDS_peptides', fa, gff, out, 'order=insertion']
    assert genome_tools.main(argv) == 0
    with open(out) as fh:
        assert fh.read() == golden['basic']['out']
    # a string of filters: every character is one
    assert genome_tools.main(argv + ['gene_name_filters=xB', 'names_from=CDS']) == 0
    with open(out) as fh:
        assert fh.read() == golden['filter_string']['out']
    assert genome_tools.main(argv + ['gene_length_filter=323']) == 0
    with open(out) as fh:
        assert fh.read() == golden['length_above']['out']
    assert genome_tools.get_CDS_peptides.last_path[1] == 'native'


def test_a_bad_integer_takes_the_object_path(inputs, tmp_path):
    fa, gff, _, _, _ = inputs['basic']
    with pytest.raises(ValueError):
        genome_tools.get_CDS_peptides(fa, gff, str(tmp_path / 'o.fa'), gene_length_filter='12x')
    assert genome_tools.get_CDS_peptides.last_path == ('get_CDS_peptides', 'host', 'bad integer')
