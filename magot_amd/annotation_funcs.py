"""annotation_funcs.py of the reference: set operations on annotations, of
which it has one, ``annotation_overlap`` (annotation_funcs.py:13-30).

The reference compares every feature of one dict with every feature of the
other.  Here the first dict's coordinates are sorted once on the device
(engine.IntervalIndex) and each feature of the second costs a few binary
searches and a scan of the intervals that start inside it.
"""

import numpy as np

from . import engine
from . import py2order


def _keys_in_order(features, order):
    """The dict's keys as the reference's Python 2 iterates them (``order='py2'``:
    a dict that ``read_gff`` built was rebuilt by each deep copy since) or as
    inserted."""
    keys = list(features)
    if order == 'insertion':
        return keys
    if order != 'py2':
        raise ValueError("order must be 'insertion' or 'py2'")
    copies = 0
    for obj in features.values():
        aset = getattr(obj, 'annotation_set', None)
        held = getattr(aset, '__dict__', {})
        if any(val is features for val in held.values()):
            copies = held.get('_magot_copies', 0)
        break
    return py2order.order_after_copies(keys, copies)


def _overlap_loop(features1, keys1, features2, keys2):
    """annotation_funcs.py:13-30 restated, over the given key orders"""
    annotation_coords_dict = {}
    contained_list = []
    for annotation in keys1:
        annotation_obj = features1[annotation]
        annotation_coords_dict.setdefault(annotation_obj.seqid, []).append(
            annotation_obj.get_coords())
    for annotation in keys2:
        annotation_obj = features2[annotation]
        seqid = annotation_obj.seqid
        coords2 = annotation_obj.get_coords()
        if seqid in annotation_coords_dict:
            for coords1 in annotation_coords_dict[seqid]:
                if (coords1[0] <= coords2[0] <= coords1[1] or
                        coords1[0] <= coords2[1] <= coords1[1]):
                    contained_list.append(annotation_obj.ID)
    return contained_list


def _columns(features, keys, seq_of, add):
    """(seqid numbers, c0, c1) of the features, get_coords() called once per
    object; None when a coordinate pair is not two integers the index holds.
    ``seq_of`` numbers the seqids; new ones are added when ``add``, else -1."""
    lo, hi = engine.IntervalIndex.coord_range()
    seq, c0, c1 = [], [], []
    for key in keys:
        obj = features[key]
        coords = obj.get_coords()
        a, b = coords[0], coords[1]
        if not (type(a) is int and type(b) is int and lo <= a <= hi and lo <= b <= hi):
            return None
        if add:
            seq.append(seq_of.setdefault(obj.seqid, len(seq_of)))
        else:
            seq.append(seq_of.get(obj.seqid, -1))
        c0.append(a)
        c1.append(b)
    return (np.asarray(seq, np.int64), np.asarray(c0, np.int64), np.asarray(c1, np.int64))


def annotation_overlap(annotation_set_features1, annotation_set_features2, order='py2',
                       native=True):
    """annotation_funcs.py:13-30: the IDs of the second feature dict (for
    example ``aset.gene``) whose features overlap one of the first on the same
    seqid, once per overlapping partner, in the second dict's iteration order.
    q overlaps p when p0 <= q0 <= p1 or p0 <= q1 <= p1 on ``get_coords()``:
    closed comparisons, and a p strictly inside q does not count.

    ``order='py2'`` iterates the second dict as the reference's Python 2 does,
    ``'insertion'`` as it was filled.  On the device (engine.IntervalIndex, the
    list expanded from the counts) unless an object's ``get_coords()`` is None
    (a parent without children), raises, or is not a pair of integers in the
    index's range: the loop restated from the reference then runs instead, so
    its exception comes out; ``native=False`` forces it.
    ``annotation_overlap.last_path`` names the path the last call took."""
    keys1 = _keys_in_order(annotation_set_features1, order)
    keys2 = _keys_in_order(annotation_set_features2, order)
    why = 'native is not True'
    if native is True:
        try:
            seq_of = {}
            first = _columns(annotation_set_features1, keys1, seq_of, True)
            second = first and _columns(annotation_set_features2, keys2, seq_of, False)
            why = None if second else 'coordinates that are not integers in range'
        except Exception:  # whatever get_coords() raises, the loop raises again
            second = None
            why = 'get_coords() is None or raises'
        if second:
            index = engine.IntervalIndex(*first, n_seq=len(seq_of))
            try:
                counts = index.overlap_counts(*second)
            finally:
                index.close()
            ids = np.empty(len(keys2), dtype=object)
            for k, key in enumerate(keys2):
                ids[k] = annotation_set_features2[key].ID
            annotation_overlap.last_path = ('annotation_overlap', 'native', None)
            return list(np.repeat(ids, counts))
    annotation_overlap.last_path = ('annotation_overlap', 'host', why)
    return _overlap_loop(annotation_set_features1, keys1, annotation_set_features2, keys2)


annotation_overlap.last_path = None
