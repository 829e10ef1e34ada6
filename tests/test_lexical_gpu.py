"""Lexical search on the GPU against its numpy restatement (tests/lexical_ref.py): scores bit for bit, rows of the exact
top-k identical in index and value.

Corpora (C = tt_lexical_chunk_docs()):
  main  N = 3 C + 17, F = 257: row lengths from {0..40}, random positive values, column 256 used by no document.  One row is
        duplicated at 1, C - 1, C, 2 C + 3 and N - 1 (its copies straddle chunks).  Three rows of 3 000 entries -- longer than
        any staging piece -- sit at a chunk's first row (2 C), last row (2 C - 1) and interior (C / 2 + 7).  At F = 257 a row
        of 3 000 entries cannot have distinct columns: these three repeat the columns 0..255 in ascending runs, which is outside
        the stated format but defined by the score contract (products in stored order), and their values are scaled by 1/64 so
        that they do not outrank the duplicated row in the tie test.  It is used through the functional forms and the C ABI.
  wide  N = C + 17, F = TT_LEXICAL_FMAX: the same short rows, and three rows of 3 000 strictly ascending entries at 0, C - 1 and
        C / 2: a valid matrix, used wherever the test goes through LexicalIndex (which validates).
  big   N = 65 C + 3, F = 257, rows of 0..8 entries: more than 64 chunks, where the partial lists are merged in two steps."""
import ctypes

import numpy as np
import pytest
import torch

import lexical_ref as ref
import poison

pytestmark = pytest.mark.gpu

F = ref.MAIN_F
TIE_COLS = ref.TIE_COLS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Corpus:
    def __init__(self, indptr, cols, vals, F):
        self.indptr, self.cols, self.vals, self.F = indptr, cols, vals, F
        self.N = indptr.size - 1
        self.t = (_dev(indptr), _dev(cols), _dev(vals))

    def scores32(self, q_cols, q_vals):
        return ref.ref_scores32(self.indptr, self.cols, self.vals, ref.dense_query(q_cols, q_vals, self.F))


@pytest.fixture(scope="module")
def env():
    import twotowermlretrieval_amd as tt
    from twotowermlretrieval_amd import _lib
    from twotowermlretrieval_amd.lexical import TT_LEXICAL_FMAX
    lib = _lib.lib()
    C = lib.tt_lexical_chunk_docs()

    class E:
        pass
    e = E()
    e.tt, e.lib, e.C, e.FMAX = tt, lib, C, TT_LEXICAL_FMAX

    # main (built in lexical_ref: test_lexical_big_gpu.py places the same corpus at high offsets of the nnz stream)
    m = ref.MainCorpus(C)
    rng = m.rng
    e.long_rows, e.tie_rows, e.tie_vals = m.long_rows, m.tie_rows, m.tie_vals
    e.main = Corpus(m.indptr, m.cols, m.vals, F)
    e.queries, e.S = m.queries, m.S
    e.batch = ("random", "every", "one")

    # wide
    Nw = C + 17
    ip, cols, vals = ref.random_corpus(2, Nw, TT_LEXICAL_FMAX, long_rows=(0, C - 1, C // 2))
    e.wide = Corpus(ip, cols, vals, TT_LEXICAL_FMAX)
    qw = rng.choice(TT_LEXICAL_FMAX, size=2000, replace=False)
    e.wide_queries = [(qw, rng.uniform(0.05, 1.0, size=qw.size).astype(np.float32)),
                      (qw[:30], rng.uniform(0.05, 1.0, size=30).astype(np.float32))]
    e.wide_S = [e.wide.scores32(*q) for q in e.wide_queries]
    return e


def _q(queries):
    return tuple(_dev(a) for a in ref.queries_csr(queries))


def _search(e, corpus, names_or_queries, k, **kw):
    qs = [e.queries[n] if isinstance(n, str) else n for n in names_or_queries]
    v, i = e.tt.lexical_score_topk(corpus.t, corpus.F, _q(qs), k, **kw)
    torch.cuda.synchronize()
    return v.cpu().numpy(), i.cpu().numpy()


def _assert_rows(got_v, got_i, want, what=""):
    for b, (wv, wi) in enumerate(want):
        assert np.array_equal(got_i[b], wi), (what, b, got_i[b][:12], wi[:12])
        assert np.array_equal(_bits(got_v[b]), _bits(wv)), (what, b)


# ---------------------------------------------------------------- score_all, bit for bit

@pytest.mark.parametrize("names", [("random",), ("empty", "one", "every"), ("tie", "nothing", "random")])
def test_score_all_bit_exact(env, names):
    S = env.tt.lexical_score_all(env.main.t, F, _q([env.queries[n] for n in names])).cpu().numpy()
    assert S.shape == (len(names), env.main.N)
    for b, n in enumerate(names):
        assert np.array_equal(_bits(S[b]), _bits(env.S[n])), n
    assert not S[names.index("empty")].any() if "empty" in names else True


def test_score_all_drops_a_query_column_outside_F_through_the_c_abi(env):
    """A column >= F (or negative) in the QUERY's list: the kernel must tolerate it, and the Python layer names it when
    asked (check_query_columns: a host read).  A search does not ask -- it stays asynchronous to the host
    (tests/test_streams_index_gpu.py) -- and returns what the kernel computes without those columns."""
    m = env.main
    q_cols = np.array([3, F, 50, F + 1000, -7, 2 ** 31 - 1], dtype=np.int32)
    q_vals = np.array([0.5, 9.0, 0.25, 9.0, 9.0, 9.0], dtype=np.float32)
    qi, qc, qv = _dev(np.array([0, q_cols.size], dtype=np.int64)), _dev(q_cols), _dev(q_vals)
    S = torch.empty((1, m.N), dtype=torch.float32, device="cuda")
    rc = env.lib.tt_lexical_score_all_f32(m.t[0].data_ptr(), m.t[1].data_ptr(), m.t[2].data_ptr(), m.N, F, qi.data_ptr(),
                                          qc.data_ptr(), qv.data_ptr(), 1, S.data_ptr(), None)
    assert rc == 0, env.lib.tt_last_error()
    torch.cuda.synchronize()
    want = m.scores32(np.array([3, 50]), np.array([0.5, 0.25], dtype=np.float32))
    assert np.array_equal(_bits(S.cpu().numpy()[0]), _bits(want))
    from twotowermlretrieval_amd.lexical import check_query_columns
    with pytest.raises(ValueError, match="column outside"):  # the Python layer refuses the same query, where it looks
        check_query_columns((qi, qc, qv), F)
    check_query_columns(_q([(np.array([3, 50]), np.array([0.5, 0.25], dtype=np.float32))]), F)
    small = Corpus(*ref.random_corpus(5, 300, F), F)  # (a valid matrix: LexicalIndex validates, `main` repeats columns)
    gv, gi = env.tt.LexicalIndex((*small.t, F)).search((qi, qc, qv), 10)  # ... and a search ranks without those columns
    torch.cuda.synchronize()
    want = small.scores32(np.array([3, 50]), np.array([0.5, 0.25], dtype=np.float32))
    _assert_rows(gv.cpu().numpy(), gi.cpu().numpy(), [ref.ref_topk(want, 10)], "columns outside F")


def test_score_all_at_fmax_with_long_sorted_rows(env):
    w = env.wide
    S = env.tt.lexical_score_all(w.t, w.F, _q(env.wide_queries)).cpu().numpy()
    for b in range(2):
        assert np.array_equal(_bits(S[b]), _bits(env.wide_S[b])), b
    assert S[0][0] > 0 and S[0][env.C - 1] > 0 and S[0][env.C // 2] > 0     # the 3 000-entry rows are hit


# ---------------------------------------------------------------- search against ref_topk

@pytest.mark.parametrize("k", [1, 10, 64, 65, 1024])
def test_search_matches_ref_topk(env, k):
    v, i = _search(env, env.main, env.batch, k)
    _assert_rows(v, i, [ref.ref_topk(env.S[n], k) for n in env.batch], f"k={k}")


@pytest.mark.parametrize("k", [10, 1024])
def test_search_at_fmax(env, k):
    v, i = _search(env, env.wide, env.wide_queries, k)
    _assert_rows(v, i, [ref.ref_topk(s, k) for s in env.wide_S], f"wide k={k}")


@pytest.mark.parametrize("k", [7, 100])
def test_k_above_n_writes_the_tail(env, k):
    m = env.main
    small = Corpus(m.indptr[:6].copy(), m.cols[:m.indptr[5]].copy(), m.vals[:m.indptr[5]].copy(), F)
    v, i = _search(env, small, ("every", "nothing"), k)
    want = [ref.ref_topk(env.S[n][:5], k) for n in ("every", "nothing")]
    _assert_rows(v, i, want)
    assert (i[:, 5:] == -1).all() and np.isneginf(v[:, 5:]).all() and (i[:, :5] >= 0).all()


def test_empty_corpus_and_empty_batch(env):
    empty = (_dev(np.zeros(1, dtype=np.int64)), _dev(np.zeros(0, dtype=np.int32)), _dev(np.zeros(0, dtype=np.float32)))
    v, i = env.tt.lexical_score_topk(empty, F, _q([env.queries["random"]]), 4)
    assert (i.cpu().numpy() == -1).all() and np.isneginf(v.cpu().numpy()).all()
    assert env.tt.lexical_score_all(empty, F, _q([env.queries["random"]])).shape == (1, 0)
    v, i = env.tt.lexical_score_topk(env.main.t, F, _q([]), 4)
    assert v.shape == (0, 4) and i.shape == (0, 4)


def test_tie_order_across_chunks(env):
    """The duplicated row is the query: its five copies score the same bits, rank first and come out in index order."""
    s = env.S["tie"]
    top = s[list(env.tie_rows)]
    assert len(set(_bits(top).tolist())) == 1 and (np.delete(s, list(env.tie_rows)) < top[0]).all()
    v, i = _search(env, env.main, ("tie",), 10)
    assert i[0][:5].tolist() == list(env.tie_rows)
    _assert_rows(v, i, [ref.ref_topk(s, 10)])
    v, i = _search(env, env.main, ("tie",), 3)
    assert i[0].tolist() == list(env.tie_rows[:3]) and np.array_equal(_bits(v[0]), _bits(top[:3]))


@pytest.mark.parametrize("k", [10, 100])
def test_all_zero_scores_return_the_first_k(env, k):
    assert not env.S["nothing"].any()
    v, i = _search(env, env.main, ("nothing", "empty"), k)
    for b in range(2):
        assert i[b].tolist() == list(range(k))
        assert (_bits(v[b]) == 0).all()                    # +0, bit for bit


def test_dyadic_corpus_agrees_exactly_in_f32_f64_and_on_the_gpu(env):
    """Values and weights are multiples of 2^-6 in (0, 1], at most 16 terms per row: every partial sum is a multiple of 2^-12
    below 16, exact in float32, so the three agree exactly."""
    rng = np.random.default_rng(5)
    N = env.C + 17
    ip, cols, _ = ref.random_corpus(3, N, F, max_len=16)
    vals = (rng.integers(1, 65, size=cols.size) / 64.0).astype(np.float32)
    c = Corpus(ip, cols, vals, F)
    qc = rng.permutation(F)[:120]
    qv = (rng.integers(1, 65, size=qc.size) / 64.0).astype(np.float32)
    s32 = c.scores32(qc, qv)
    s64 = ref.ref_scores64(ip, cols, vals, ref.dense_query(qc, qv, F))
    assert np.array_equal(s32.astype(np.float64), s64)
    S = env.tt.lexical_score_all(c.t, F, _q([(qc, qv)])).cpu().numpy()[0]
    assert np.array_equal(S.astype(np.float64), s64) and np.array_equal(_bits(S), _bits(s32))
    v, i = _search(env, c, [(qc, qv)], 50)
    _assert_rows(v, i, [ref.ref_topk(s32, 50)])           # dyadic scores tie often: the order is by index


# ---------------------------------------------------------------- keep, min_score, base

def test_keep_mask(env):
    m, tt = env.main, env.tt
    s = env.S["random"]
    _, best = ref.ref_topk(s, 3)
    keep = np.ones(m.N, dtype=bool)
    keep[best[0]] = False
    keep[np.arange(5, m.N, 7)] = False
    keep[best[1]] = True
    for k in (10, 100):
        v, i = _search(env, m, ("random",), k, keep=tt.pack_keep_mask(_dev(keep)))
        assert best[0] not in i[0] and i[0][0] == best[1]                  # removed: never returned; the next one is promoted
        _assert_rows(v, i, [ref.ref_topk(s, k, keep=keep)])
    v, i = _search(env, m, ("random", "every"), 10, keep=tt.pack_keep_mask(_dev(np.zeros(m.N, dtype=bool))))
    assert (i == -1).all() and np.isneginf(v).all()                         # a mask that keeps nothing: empty rows


def test_remove_ids_equals_keep(env):
    w, tt = env.wide, env.tt
    off = 1000
    ix = tt.LexicalIndex((*w.t, w.F), idx_offset=off)
    assert ix.ntotal == w.N and ix.n_features == w.F and ix.device.type == "cuda" and ix.keep_mask is None
    q = _q(env.wide_queries)
    _, best = ref.ref_topk(env.wide_S[0], 4)
    gone = [int(best[0]), int(best[2]), 0, w.N - 1]
    keep = np.ones(w.N, dtype=bool)
    keep[gone] = False
    v0, i0 = ix.search(q, 20, keep=tt.pack_keep_mask(_dev(keep)))
    ix.remove_ids([g + off for g in gone] + [5, off + w.N + 3])             # ids that are not this index's are ignored
    v1, i1 = ix.search(q, 20)
    assert torch.equal(i0, i1) and torch.equal(v0.view(torch.int32), v1.view(torch.int32))
    want = [ref.ref_topk(s, 20, keep=keep, idx_offset=off) for s in env.wide_S]
    _assert_rows(v1.cpu().numpy(), i1.cpu().numpy(), want)
    assert ix.keep_mask is not None and ix.score_all(q).shape == (2, w.N)


def test_min_score(env):
    m = env.main
    attained = float(ref.ref_topk(env.S["random"], 7)[0][6])                # the 7th best score of query 0: >= keeps it
    thr = np.array([attained, np.inf, 0.5], dtype=np.float32)
    v, i = _search(env, m, env.batch, 10, min_score=_dev(thr))
    want = [ref.ref_topk(env.S[n], 10, min_score=t) for n, t in zip(env.batch, thr)]
    _assert_rows(v, i, want)
    n_at = int((env.S["random"] >= np.float32(attained)).sum())
    assert 7 <= n_at < 10 and (i[0][:n_at] >= 0).all() and (i[0][n_at:] == -1).all() and v[0][n_at - 1] == np.float32(attained)
    assert (i[1] == -1).all() and np.isneginf(v[1]).all()                   # +inf: an empty row
    v, i = _search(env, m, env.batch, 100, min_score=1e-5)                  # one number for every query
    _assert_rows(v, i, [ref.ref_topk(env.S[n], 100, min_score=np.float32(1e-5)) for n in env.batch])


def test_base_blend(env):
    m = env.main
    rng = np.random.default_rng(9)
    wide = rng.standard_normal((3, m.N + 13)).astype(np.float32)
    base = _dev(wide)[:, :m.N]                                              # row stride N + 13 > N
    assert base.stride(0) == m.N + 13
    vals = [ref.blend32(wide[b, :m.N], env.S[n], 0.3, 0.7) for b, n in enumerate(env.batch)]
    for k in (10, 100):
        v, i = _search(env, m, env.batch, k, base=base, w_base=0.3, w_lex=0.7)
        _assert_rows(v, i, [ref.ref_topk(x, k) for x in vals], f"base k={k}")
    keep = rng.random(m.N) < 0.5
    v, i = _search(env, m, env.batch, 10, base=base, w_base=0.3, w_lex=0.7, keep=env.tt.pack_keep_mask(_dev(keep)),
                   min_score=0.25)
    _assert_rows(v, i, [ref.ref_topk(x, 10, keep=keep, min_score=0.25) for x in vals])


# ---------------------------------------------------------------- slices, workspace, graph, many chunks

@pytest.mark.parametrize("k", [10, 100])
def test_slices_merge_to_the_whole_corpus_search(env, k):
    m, tt, r = env.main, env.tt, env.C + 5
    q = _q([env.queries[n] for n in env.batch])
    ip, cols, vals = m.t
    va, ia = tt.lexical_score_topk((ip[:r + 1], cols, vals), F, q, k)
    vb, ib = tt.lexical_score_topk((ip[r:], cols, vals), F, q, k, idx_offset=r)
    assert int(ia.max()) < r <= int(ib[ib >= 0].min())
    v, i = tt.topk_merge(torch.cat([va, vb], 1), torch.cat([ia, ib], 1), k)
    vw, iw = tt.lexical_score_topk(m.t, F, q, k)
    assert torch.equal(i, iw) and torch.equal(v.view(torch.int32), vw.view(torch.int32))
    _assert_rows(v.cpu().numpy(), i.cpu().numpy(), [ref.ref_topk(env.S[n], k) for n in env.batch])


@pytest.mark.parametrize("k", [10, 100])
def test_result_does_not_depend_on_what_workspace_and_outputs_held(env, k):
    got = []
    for word in (0xFFFFFFFF, 0x00000000):
        with poison.poisoned_empty(word) as p:
            v, i = env.tt.lexical_score_topk(env.main.t, F, _q([env.queries[n] for n in env.batch]), k,
                                             keep=env.tt.pack_keep_mask(_dev(np.arange(env.main.N) % 3 != 0)))
        assert p.tensors >= 3                               # the two outputs and the workspace at least
        got.append((v.cpu().numpy(), i.cpu().numpy()))
    assert np.array_equal(_bits(got[0][0]), _bits(got[1][0])) and np.array_equal(got[0][1], got[1][1])
    keep = np.arange(env.main.N) % 3 != 0
    _assert_rows(*got[0], [ref.ref_topk(env.S[n], k, keep=keep) for n in env.batch])


def test_graph_replay_with_queries_changed_in_place(env):
    w, tt = env.wide, env.tt
    ix = tt.LexicalIndex((*w.t, w.F))
    cap = 64
    qi = torch.zeros(2, dtype=torch.int64, device="cuda")
    qc = torch.zeros(cap, dtype=torch.int32, device="cuda")
    qv = torch.zeros(cap, dtype=torch.float32, device="cuda")
    out = (torch.empty((1, 10), dtype=torch.float32, device="cuda"), torch.empty((1, 10), dtype=torch.int64, device="cuda"))

    def put(cols, vals):
        qc[:len(cols)].copy_(_dev(np.asarray(cols, dtype=np.int32)))
        qv[:len(cols)].copy_(_dev(np.asarray(vals, dtype=np.float32)))
        qi.copy_(_dev(np.array([0, len(cols)], dtype=np.int64)))

    put(*[a[:30] for a in env.wide_queries[1]])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ix.search((qi, qc, qv), 10, out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ix.search((qi, qc, qv), 10, out=out)
    rng = np.random.default_rng(21)
    for m in (64, 5):
        cols = rng.choice(w.F, size=m, replace=False)
        vals = rng.uniform(0.05, 1.0, size=m).astype(np.float32)
        put(cols, vals)
        out[0].fill_(7.0)
        out[1].fill_(7)
        g.replay()
        torch.cuda.synchronize()
        dv, di = ix.search(_q([(cols, vals)]), 10)
        assert torch.equal(out[1], di) and torch.equal(out[0].view(torch.int32), dv.view(torch.int32))
        _assert_rows(out[0].cpu().numpy(), out[1].cpu().numpy(), [ref.ref_topk(w.scores32(cols, vals), 10)])


@pytest.fixture(scope="module")
def big(env):
    """More than 64 chunks: rows of 0..8 entries, columns = running sums of steps in 1..30 (ascending, below 241)."""
    rng = np.random.default_rng(31)
    N = 65 * env.C + 3
    lens = rng.integers(0, 9, size=N)
    allc = np.cumsum(rng.integers(1, 31, size=(N, 8)), axis=1) - 1
    take = np.arange(8)[None, :] < lens[:, None]
    indptr = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    cols = allc[take].astype(np.int32)
    vals = (rng.integers(1, 9, size=cols.size) / 8.0).astype(np.float32)     # few distinct values: large tie groups
    c = Corpus(indptr, cols, vals, F)
    qc = rng.permutation(241)[:40]
    qv = (rng.integers(1, 5, size=40) / 4.0).astype(np.float32)
    return c, (qc, qv), c.scores32(qc, qv)


@pytest.mark.parametrize("k", [10, 64, 100, 1024])
def test_many_chunks_two_step_merge(env, big, k):
    c, q, s = big
    assert c.N > 64 * env.C
    with poison.poisoned_empty(0xFFFFFFFF):
        v, i = env.tt.lexical_score_topk(c.t, F, _q([q, env.queries["nothing"]]), k)
    _assert_rows(v.cpu().numpy(), i.cpu().numpy(), [ref.ref_topk(s, k), ref.ref_topk(np.zeros(c.N, np.float32), k)])


def test_c_abi_direct_call_with_idx_offset(env):
    """The raw entry point as a ctypes caller binds it: sizes from the workspace query, idx_offset added to every index."""
    m, lib = env.main, env.lib
    qi, qc, qv = _q([env.queries["random"]])
    k, off = 10, 1 << 40
    need = lib.tt_lexical_workspace_bytes(1, m.N, k)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ov = torch.empty((1, k), dtype=torch.float32, device="cuda")
    oi = torch.empty((1, k), dtype=torch.int64, device="cuda")
    args = [m.t[0].data_ptr(), m.t[1].data_ptr(), m.t[2].data_ptr(), m.N, F, qi.data_ptr(), qc.data_ptr(), qv.data_ptr(), 1,
            None, None, None, 0, 0.0, 1.0, k, off, ov.data_ptr(), oi.data_ptr(), ws.data_ptr()]
    assert lib.tt_lexical_score_topk_f32(*args, need - 1, None) == 5          # TT_ERR_WORKSPACE, nothing launched
    assert lib.tt_lexical_score_topk_f32(*args, need, None) == 0, lib.tt_last_error()
    torch.cuda.synchronize()
    _assert_rows(ov.cpu().numpy(), oi.cpu().numpy(), [ref.ref_topk(env.S["random"], k, idx_offset=off)])
    assert isinstance(ctypes.c_void_p(ws.data_ptr()).value, int)
