"""CPU restatement (numpy) of the hand-over of include/singa_hip_stream.h - continuous sampling: a row that has ended its
molecule starts the pocket's next one.  The rule moves rows step by step; this restatement does not: a row is busy for as
many steps as its molecule has tokens, so the order in which rows fall free is known from the step counts alone, and the
pocket's molecules are handed out to the rows by an event queue (free step, row) in which ties go to the lower row."""
import heapq

import numpy as np


def stream_rule(counts, rows_per_pocket):
    """counts [pockets, num_samples] int: the steps every molecule takes (its tokens, the '$' included; >= 1).  Returns
    (row_of [pockets * num_samples] int32 - rows are pocket-major, `rows_per_pocket` per pocket -, start_step [same] int32,
    the steps of the whole run)."""
    counts = np.asarray(counts)
    B, n = counts.shape
    assert (counts >= 1).all()
    R = int(rows_per_pocket)
    row_of, start = np.zeros((B, n), np.int32), np.zeros((B, n), np.int32)
    total = 0
    for b in range(B):
        free = [(0, i) for i in range(min(R, n))]              # (the step at which the row takes its next molecule, row)
        heapq.heapify(free)
        for j in range(n):
            s, i = heapq.heappop(free)
            row_of[b, j], start[b, j] = b * R + i, s
            heapq.heappush(free, (s + int(counts[b, j]), i))
            total = max(total, s + int(counts[b, j]))
    return row_of.reshape(-1), start.reshape(-1), total


def live_after(counts, rows_per_pocket, steps):
    """Rows of every pocket that hold a molecule after `steps` steps of the run -> [pockets] int: the molecules that have been
    handed out (start_step <= steps: one handed over in step s starts in step s + 1) and have not ended."""
    counts = np.asarray(counts)
    start = stream_rule(counts, rows_per_pocket)[1].reshape(counts.shape)
    return ((start <= steps) & (start + counts > steps)).sum(1)
