"""include/memb_hip_within.h restated by a plain loop, sharing no code with memb_amd.reader.within_host: per row every
column that is not named goes, together with the mark, into ONE list that `sorted` puts into the selection's order (key
descending, position ascending); what stands before the mark is the row's list, given back in ascending position."""
import numpy as np

from ranks_reference import key_of


def within_by_the_contract(matrix, thresholds, marks, base=0, exclude=None):
    """(offsets int64 (Q + 1,), positions int64 (total,), values float32 (total,)) of the float32 (Q, n) matrix, a column
    c being the position base + c"""
    matrix = np.asarray(matrix, dtype=np.float32)
    count, n = matrix.shape
    offsets, positions, bits = [0], [], []
    for q in range(count):
        dropped = set() if exclude is None else {int(entry) for entry in exclude[q]}
        # (the mark's position cut to base - 1 .. base + n: its place among the columns' positions stays; among entries
        # with its key AND position the mark comes first, since such an entry does not precede it)
        mark = (-key_of(thresholds[q]), min(max(int(marks[q]), base - 1), base + n), 0, None)
        entries = [(-key_of(matrix[q, c]), base + c, 1, c) for c in range(n) if base + c not in dropped]
        ordered = sorted(entries + [mark])
        before = sorted(entry[3] for entry in ordered[:ordered.index(mark)])
        positions += [base + c for c in before]
        bits += [int(matrix[q, c:c + 1].view(np.uint32)[0]) for c in before]
        offsets.append(len(positions))
    return (np.array(offsets, dtype=np.int64), np.array(positions, dtype=np.int64),
            np.array(bits, dtype=np.uint32).view(np.float32))


def same_lists(got, want):
    """both (offsets, positions, values): equal integers and equal BITS"""
    return (got[0].tolist() == want[0].tolist() and got[1].tolist() == want[1].tolist() and
            np.ascontiguousarray(got[2]).view(np.uint32).tolist() == np.ascontiguousarray(want[2]).view(np.uint32).tolist())
