"""numpy reference of the device graph builder (gatv2_abi.h "graph construction"): the definition restated, nothing shared
with the library.  Edges (src[i], dst[i]), message src -> dst; dst a row of the context, src a row of the source table."""
import numpy as np

SELF_LOOPS, SYMMETRIZE, COALESCE = 1, 2, 4


def graph_ref(src, dst, n_rows, n_table=None, table_row0=0, flags=0):
    """-> (row_ptr int32 [n_rows+1], col_idx int32): rows = destinations, sources ascending inside a row.
    Order of application: symmetrize, self-loops (drop every existing one, add exactly one per row), coalesce."""
    n_table = n_rows if n_table is None else n_table
    s, d = np.asarray(src, np.int64), np.asarray(dst, np.int64)
    assert len(s) == len(d) and (len(s) == 0 or (s.min() >= 0 and s.max() < n_table and d.min() >= 0 and d.max() < n_rows))
    if flags & SYMMETRIZE:
        assert n_table == n_rows and table_row0 == 0
        off = s != d
        s, d = np.concatenate([s, d[off]]), np.concatenate([d, s[off]])
    if flags & SELF_LOOPS:
        keep = s != table_row0 + d
        r = np.arange(n_rows, dtype=np.int64)
        s, d = np.concatenate([s[keep], table_row0 + r]), np.concatenate([d[keep], r])
    if flags & COALESCE:
        pairs = np.unique(np.stack([d, s], 1), axis=0) if len(s) else np.zeros((0, 2), np.int64)
        d, s = pairs[:, 0], pairs[:, 1]
    order = np.lexsort((s, d))                     # by destination, then source
    row_ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(d, minlength=n_rows), out=row_ptr[1:])
    return row_ptr.astype(np.int32), s[order].astype(np.int32)


def csr_to_coo(row_ptr, col_idx):
    """(src, dst) of a CSR whose rows are destinations."""
    return np.asarray(col_idx, np.int32), np.repeat(np.arange(len(row_ptr) - 1, dtype=np.int32), np.diff(row_ptr))
