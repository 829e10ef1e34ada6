"""numpy restatement of the lexical search contract (include/tt.h "Lexical search"), for the tests.

    s(b,n) = ((0 + p_1) + p_2) + ...,   p_i = fl32(vals[i] * q_b[cols[i]])   over row n's entries in stored order

ref_scores32 is that chain in np.float32 -- the bit-exact yardstick --, ref_scores64 the same dot product in float64, and
ref_topk the selection: (value desc, index asc) among the kept documents whose value is >= min_score, NaN never."""
import numpy as np


def dense_query(q_cols, q_vals, F):
    """The dense image of one sparse query; columns outside [0, F) are dropped, as the kernel's guard drops them."""
    q = np.zeros(F, dtype=np.float32)
    c = np.asarray(q_cols, dtype=np.int64)
    ok = (c >= 0) & (c < F)
    q[c[ok]] = np.asarray(q_vals, dtype=np.float32)[ok]
    return q


def _chain(indptr, prod, dtype):
    """Per row, the sequential sum of prod[indptr[n] : indptr[n+1]] in `dtype`, in stored order, from +0."""
    indptr = np.asarray(indptr, dtype=np.int64)
    lens = np.diff(indptr)
    acc = np.zeros(lens.size, dtype=dtype)
    rows = np.arange(lens.size)
    j = 0
    while rows.size:
        rows = rows[lens[rows] > j]  # rows that still have a j-th entry
        acc[rows] = (acc[rows] + prod[indptr[rows] + j]).astype(dtype)
        j += 1
    return acc


def ref_scores32(indptr, cols, vals, q):
    """q: dense float32 [F].  The product array is rounded to float32 first, then added one by one in float32."""
    q = np.asarray(q, dtype=np.float32)
    cols = np.asarray(cols, dtype=np.int64)
    ok = (cols >= 0) & (cols < q.size)
    w = np.where(ok, q[np.where(ok, cols, 0)], np.float32(0)).astype(np.float32)
    prod = np.where(ok, np.asarray(vals, dtype=np.float32) * w, np.float32(0)).astype(np.float32)
    return _chain(indptr, prod, np.float32)


def ref_scores64(indptr, cols, vals, q):
    q = np.asarray(q, dtype=np.float64)
    cols = np.asarray(cols, dtype=np.int64)
    ok = (cols >= 0) & (cols < q.size)
    prod = np.where(ok, np.asarray(vals, dtype=np.float64) * q[np.where(ok, cols, 0)], 0.0)
    return _chain(indptr, prod, np.float64)


def ref_topk(values, k, keep=None, min_score=None, idx_offset=0):
    """values float32 [N] -> (vals float32 [k], idx int64 [k]): stable argsort of the negated values = (value desc, index
    asc); keep: bool [N] or None; the tail is (-inf, -1).  -0 ranks as +0 (the sort compares them equal) and is returned as +0;
    a -inf value is a candidate like any other (only min_score can exclude it) and ranks after every finite one."""
    values = np.asarray(values, dtype=np.float32)
    cand = ~np.isnan(values)
    if keep is not None:
        cand &= np.asarray(keep, dtype=bool)
    if min_score is not None:
        with np.errstate(invalid="ignore"):
            cand &= values >= np.float32(min_score)
    ids = np.nonzero(cand)[0]
    order = ids[np.argsort(-values[ids], kind="stable")][:k]
    out_v = np.full(k, -np.inf, dtype=np.float32)
    out_i = np.full(k, -1, dtype=np.int64)
    out_v[:order.size] = values[order] + np.float32(0)     # "a zero value is returned as +0": -0 + 0 = +0, all else unchanged
    out_i[:order.size] = order + idx_offset
    return out_v, out_i


def blend32(base, s, w_base, w_lex):
    """The ranked value with a base: fl32(fl32(w_base * base) + fl32(w_lex * s)), three roundings."""
    a = (np.float32(w_base) * np.asarray(base, dtype=np.float32)).astype(np.float32)
    b = (np.float32(w_lex) * np.asarray(s, dtype=np.float32)).astype(np.float32)
    return (a + b).astype(np.float32)


def random_corpus(seed, N, F, max_len=40, long_rows=(), long_len=3000, cols_below=None, signed=False):
    """CSR with row lengths drawn from {0..max_len}, strictly ascending columns below `cols_below` (default F) and random
    positive float32 values (signed=True: a random sign on each, drawn after everything else).  long_rows get long_len
    entries: strictly ascending when they fit below cols_below, otherwise
    ascending runs 0, 1, .., cols_below - 1 repeated (columns repeat: outside the stated format, but the score contract --
    the products in stored order -- defines it, and it is the only way past a staging piece at a small F)."""
    rng = np.random.default_rng(seed)
    hi = F if cols_below is None else cols_below
    lens = rng.integers(0, min(max_len, hi) + 1, size=N)
    for r in long_rows:
        lens[r] = long_len
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    cols = np.empty(int(indptr[-1]), dtype=np.int32)
    for n in range(N):
        m = int(lens[n])
        if m <= hi:
            cols[indptr[n]:indptr[n + 1]] = np.sort(rng.choice(hi, size=m, replace=False))
        else:
            cols[indptr[n]:indptr[n + 1]] = np.arange(m) % hi
    vals = rng.uniform(0.01, 1.0, size=cols.size).astype(np.float32)
    if signed:
        vals = np.where(rng.random(cols.size) < 0.5, -vals, vals).astype(np.float32)
    return indptr, cols, vals


def replace_rows(indptr, cols, vals, new_rows):
    """CSR with the rows in new_rows {row: (cols, vals)} replaced."""
    N = indptr.size - 1
    lens = np.diff(indptr)
    for r, (c, _) in new_rows.items():
        lens[r] = len(c)
    out_ip = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lens, out=out_ip[1:])
    out_c = np.empty(int(out_ip[-1]), dtype=np.int32)
    out_v = np.empty(int(out_ip[-1]), dtype=np.float32)
    for n in range(N):
        if n in new_rows:
            out_c[out_ip[n]:out_ip[n + 1]], out_v[out_ip[n]:out_ip[n + 1]] = new_rows[n]
        else:
            out_c[out_ip[n]:out_ip[n + 1]] = cols[indptr[n]:indptr[n + 1]]
            out_v[out_ip[n]:out_ip[n + 1]] = vals[indptr[n]:indptr[n + 1]]
    return out_ip, out_c, out_v


MAIN_F = 257
TIE_COLS = np.array([3, 17, 40, 41, 77, 101, 130, 131, 200, 222, 240, 255], dtype=np.int32)


class MainCorpus:
    """The `main` corpus of test_lexical_gpu.py and its queries (C = tt_lexical_chunk_docs()): N = 3 C + 17, F = 257, rows of
    0..40 entries, column 256 used by no document; three rows of 3 000 entries (values scaled by 1/64) at a chunk's first row
    (2 C), last row (2 C - 1) and interior (C / 2 + 7); one row duplicated at 1, C - 1, C, 2 C + 3 and N - 1.  S[name] are
    the float32 reference scores of queries[name], computed once and never written to.  rng: the generator, as the
    construction left it (for callers that go on drawing from it)."""

    def __init__(self, C):
        F = self.F = MAIN_F
        rng = self.rng = np.random.default_rng(11)
        N = self.N = 3 * C + 17
        self.long_rows = (2 * C, 2 * C - 1, C // 2 + 7)
        self.tie_rows = (1, C - 1, C, 2 * C + 3, N - 1)
        ip, cols, vals = random_corpus(1, N, F, long_rows=self.long_rows, cols_below=F - 1)
        for r in self.long_rows:
            vals[ip[r]:ip[r + 1]] *= np.float32(1.0 / 64)
        self.tie_vals = rng.uniform(0.5, 1.0, size=TIE_COLS.size).astype(np.float32)
        self.indptr, self.cols, self.vals = replace_rows(ip, cols, vals, {r: (TIE_COLS, self.tie_vals) for r in self.tie_rows})
        assert int(np.diff(self.indptr).max()) == 3000 and int(np.diff(self.indptr).min()) == 0 and int(self.cols.max()) == F - 2
        qa = rng.choice(F - 1, size=20, replace=False)
        self.queries = {
            "random": (qa, rng.uniform(0.05, 1.0, size=20).astype(np.float32)),
            "every": (rng.permutation(F), rng.uniform(0.05, 1.0, size=F).astype(np.float32)),
            "one": (np.array([17]), np.array([0.75], dtype=np.float32)),
            "empty": (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)),
            "nothing": (np.array([F - 1]), np.array([1.0], dtype=np.float32)),      # the column no document uses
            "tie": (TIE_COLS, self.tie_vals),
        }
        self.S = {}
        for name, q in self.queries.items():
            self.S[name] = ref_scores32(self.indptr, self.cols, self.vals, dense_query(*q, F))
            self.S[name].setflags(write=False)


def same_bits(got, want):
    """float32 arrays equal bit for bit, except that a NaN matches any NaN at the same position."""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


def queries_csr(queries):
    """[(cols, vals), ...] -> (q_indptr int64 [B+1], q_cols int32, q_vals float32)."""
    q_indptr = np.zeros(len(queries) + 1, dtype=np.int64)
    np.cumsum([len(c) for c, _ in queries], out=q_indptr[1:])
    q_cols = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in queries] + [np.zeros(0, np.int32)])
    q_vals = np.concatenate([np.asarray(v, dtype=np.float32) for _, v in queries] + [np.zeros(0, np.float32)])
    return q_indptr, q_cols.astype(np.int32), q_vals.astype(np.float32)
