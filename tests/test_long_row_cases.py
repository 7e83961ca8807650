"""What the patterns of long_row_cases.py are for: the (chunk, row, slot) table of each, recomputed here in NumPy from the long-row
rule as DESIGN.md section 3 states it, uses every slot of a chunk (nine_hubs) and several chunks per row (three_chunk_hub).  No GPU."""
import numpy as np

from long_row_cases import nine_hubs, three_chunk_hub

LONG_ROW, LONG_CHUNK, LONG_SLOTS = 512, 2048, 5


def slot_table(rowptr):
    """[(chunk, row, slot)] of every piece of a long row, in (chunk, row) order."""
    table = []
    for row in np.flatnonzero(np.diff(rowptr) > LONG_ROW):
        start, end = int(rowptr[row]), int(rowptr[row + 1])
        for chunk in range(start // LONG_CHUNK, (end - 1) // LONG_CHUNK + 1):
            c0 = chunk * LONG_CHUNK
            table.append((chunk, int(row), 0 if start < c0 else 1 + (start - c0) // LONG_ROW))
    return sorted(table)


def _checked(rowptr, col):
    """The table of a pattern, after the properties every pattern has: sorted rows, slots in range, one long row per (chunk, slot)."""
    assert rowptr[0] == 0 and rowptr[-1] == len(col)
    table = slot_table(rowptr)
    assert all(0 <= s < LONG_SLOTS for _, _, s in table)
    assert len({(c, s) for c, _, s in table}) == len(table), "two long rows of a chunk share a slot"
    return table


def test_nine_hubs_fill_every_slot():
    rowptr, col = nine_hubs()
    N, deg = len(rowptr) - 1, np.diff(rowptr)
    assert N == 600 and len(col) == 9888
    assert (deg[:9] == 521).all() and deg[9:].max() <= 10 and deg.min() >= 1
    src = np.repeat(np.arange(N), deg)
    assert np.array_equal(np.unique(src.astype(np.int64) * N + col), np.unique(col.astype(np.int64) * N + src)), "its own transpose"
    table = _checked(rowptr, col)
    assert [(r, s) for c, r, s in table if c == 0] == [(0, 1), (1, 2), (2, 3), (3, 4)]
    assert [(r, s) for c, r, s in table if c == 1] == [(3, 0), (4, 1), (5, 2), (6, 3), (7, 4)]      # every slot of one chunk
    assert [(r, s) for c, r, s in table if c == 2] == [(7, 0), (8, 1)]
    assert max(c for c, _, _ in table) == 2


def test_three_chunk_hub_spans_three_chunks():
    rowptr, col = three_chunk_hub()
    deg = np.diff(rowptr)
    assert len(rowptr) - 1 == 4500 and int(deg.argmax()) == 7 and deg[7] >= 4097
    table = _checked(rowptr, col)
    assert {r for _, r, _ in table} == {7}, "one long row"
    chunks = [c for c, _, _ in table]
    assert len(chunks) == 3 and chunks == list(range(chunks[0], chunks[0] + 3))
    assert [s for _, _, s in table][1:] == [0, 0]      # the later chunks are run into
