"""Host-side invariant of ops' packed-weight tables (ops._ROW: row-block / tile GEMM fragments, ops._FFN: fused feed-forward
W1 / W2), checked by the GPU tests after a mutation of the weights and BEFORE the next launch that can refresh a table.

A refresh launch - eager or replayed from a captured graph - reads every row that is not neutralised (source pointer 0).  Such a
row must therefore name the CURRENT storage of a live owner: a row left at the address of freed storage (an owner that died, or a
live Parameter re-pointed by `p.data = ...`) is a read of freed memory, and a GPU memory fault once that memory is unmapped
(torch.cuda.empty_cache).  Checking the table here turns that fault into a host assertion."""
from openeat_amd import ops


def _rows_by_index(tab):
    return {i: k for k, i in tab.rows.items()}


def assert_pack_rows_live():
    """Every live row of both tables names the current device address of a live owner."""
    bad = []
    for name, tab in (("_ROW", ops._ROW), ("_FFN", ops._FFN)):
        if tab.host is None:
            continue
        keys = _rows_by_index(tab)
        for i in range(tab.n):
            row = [int(v) for v in tab.host[i]]
            if row[0] == 0:
                continue                                    # neutralised: the kernel skips it
            key = keys.get(i)
            if key is None:
                bad.append((name, i, "row not neutralised but has no entry"))
                continue
            ent = tab.entries[key]
            if name == "_ROW":
                o = ent["owner"]()
                if o is None:
                    bad.append((name, i, "owner is dead"))
                elif not (o.data_ptr() <= row[0] < o.data_ptr() + o.numel() * o.element_size()):
                    bad.append((name, i, f"source {row[0]:#x} outside the owner's storage at {o.data_ptr():#x}"))
            else:
                w1, w2 = ent["w1"](), ent["w2"]()
                if w1 is None or w2 is None:
                    bad.append((name, i, "W1 or W2 is dead"))
                elif (row[0], row[1]) != (w1.data_ptr(), w2.data_ptr()):
                    bad.append((name, i, f"sources {row[0]:#x} / {row[1]:#x} are not W1 / W2 at {w1.data_ptr():#x} / {w2.data_ptr():#x}"))
    assert not bad, f"pack-table rows that a refresh launch would read from freed storage: {bad[:8]}"
