"""bench.py's host-side record keeping, on CPU: the amd-smi fields of the box
record (parsed from a metric dump a GPU box wrote in round 3, kept as
tests/data/amd_smi_metric_r03.txt) and
the counter deltas over the timed region."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMP = os.path.join(ROOT, 'tests', 'data', 'amd_smi_metric_r03.txt')


def test_smi_fields_parse_a_real_dump():
    import bench
    text = open(DUMP).read()
    got = {}
    for key, pat in bench._SMI_FIELDS:
        m = re.search(pat, text)
        if m:
            got[key] = float(m.group(1))
    assert got['used_vram_mb'] == 225420        # the other tenant's memory, round 3
    assert got['ppt_acc'] == 3788151
    assert got['mem_clk_mhz'] == 2000 and got['fclk_mhz'] == 1250
    assert got['mem_temp_c'] == 34 and got['hotspot_c'] == 47
    assert got['socket_power_w'] == 261


def test_box_state_deltas():
    import bench
    a = {'t': 1.0, 'ppt_acc': 10.0, 'energy_j': 5.0, 'used_vram_mb': 3.0}
    b = {'t': 3.5, 'ppt_acc': 16.0, 'energy_j': 9.0, 'used_vram_mb': 7.0}
    st = bench.box_state(0, a, b, {'store_gbs': 1.0}, {'store_gbs': 2.0})
    assert st['delta'] == {'t': 2.5, 'ppt_acc': 6.0, 'energy_j': 4.0}
    assert st['probe_before'] == {'store_gbs': 1.0}
    assert bench.box_state(0, None, b, None, None) == {'probe_before': None, 'probe_after': None}


def test_dump_sampling_is_fixed_and_bounded(monkeypatch):
    """--dump-outputs: small outputs whole, large ones as the same seeded
    sample every time, with block sums that cover every byte."""
    import numpy as np

    import bench
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 1000)
    monkeypatch.setattr(bench, 'DUMP_BLOCKS', 16)
    monkeypatch.setattr(bench, 'DUMP_TABLE', 100)
    a = (np.arange(5003) % 251).astype(np.uint8)
    small, big, again = {}, {}, {}
    bench._dump_bytes(small, 'x', a[:1000])
    assert list(small) == ['x'] and small['x'].dtype == np.float32
    assert np.array_equal(small['x'], a[:1000])
    bench._dump_bytes(big, 'x', a)
    bench._dump_bytes(again, 'x', a)
    assert big['x'].shape == (1000,) and np.array_equal(big['x'], again['x'])
    assert big['x_blocksum'].dtype == np.float64 and big['x_blocksum'].shape == (16,)
    assert big['x_blocksum'].sum() == a.astype(np.int64).sum()
    b = a.copy()
    b[4321] ^= 1     # one byte anywhere shows in the block sums
    other = {}
    bench._dump_bytes(other, 'x', b)
    assert not np.array_equal(other['x_blocksum'], big['x_blocksum'])
    t = np.arange(10, 1010, dtype=np.uint64) << np.uint64(40)
    assert np.array_equal(bench._dump_table(t[:100]), t[:100].astype(np.float64))
    s = bench._dump_table(t)
    assert s.dtype == np.float64 and s.shape == (100,) and np.array_equal(s, bench._dump_table(t))
    assert np.all(np.diff(s) >= 0) and set(s.tolist()) <= set(t.astype(np.float64).tolist())
