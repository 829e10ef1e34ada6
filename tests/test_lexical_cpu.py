"""Lexical search without a GPU: the four exports exist in the header, the binding table and the library; the size queries
answer; every argument check of tt_lexical_score_topk_f32 returns its status before any HIP call; the host-side builder of
LexicalIndex sorts, sums duplicates, widens indptr and validates; the product refuses CPU tensors.  Last, the float64 bound
that makes the GPU path opt-in is checked against sklearn itself."""
import ctypes
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import lexical_ref as ref

NAMES = ("tt_lexical_chunk_docs", "tt_lexical_workspace_bytes", "tt_lexical_score_topk_f32", "tt_lexical_score_all_f32")
P = 0x10000  # a well-aligned address that is never dereferenced: every check below fails before a launch


@pytest.fixture(scope="module")
def libtt():
    from twotowermlretrieval_amd import build, _lib
    build.build()
    return _lib.lib()


def _header_define(name):
    text = (ROOT / "include" / "tt.h").read_text()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", text).group(1))


def test_names_in_header_binding_table_and_library(libtt):
    from twotowermlretrieval_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "tt.h").read_text(), flags=re.S)
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(libtt, name), name
    from twotowermlretrieval_amd import lexical
    assert lexical.TT_LEXICAL_FMAX == _header_define("TT_LEXICAL_FMAX") >= 20000


def test_size_queries_need_no_gpu(libtt):
    C = libtt.tt_lexical_chunk_docs()
    assert C >= 64 and C % 64 == 0
    kmax = _header_define("TT_TOPK_LARGE_KMAX")
    one = libtt.tt_lexical_workspace_bytes(1, C, 10)
    assert one >= 10 * 12
    assert libtt.tt_lexical_workspace_bytes(1, 3 * C + 17, 10) >= 4 * 10 * 12   # one list of k (value, index) per chunk
    assert libtt.tt_lexical_workspace_bytes(3, C, 10) >= 3 * 10 * 12
    assert libtt.tt_lexical_workspace_bytes(1, 10_000_000, kmax) >= (10_000_000 // C) * kmax * 12
    assert libtt.tt_lexical_workspace_bytes(1, 0, 10) > 0                        # N = 0 still writes the tail through a list
    for bad in ((0, C, 10), (1, -1, 10), (1, C, 0), (1, C, kmax + 1), (1, 2 ** 31 - 64, 10)):
        assert libtt.tt_lexical_workspace_bytes(*bad) == 0, bad


def _topk(libtt, *, indptr=P, N=100, F=257, k=10, ws=P, ws_bytes=None, out_idx=P, out_val=P, B=1):
    if ws_bytes is None:
        ws_bytes = libtt.tt_lexical_workspace_bytes(B, N, k) if 0 < k <= 1024 else 1 << 20
    return libtt.tt_lexical_score_topk_f32(indptr, P, P, N, F, P, P, P, B, None, None, None, 0, 0.0, 1.0, k, 0, out_val, out_idx,
                                           ws, ws_bytes, None)


def test_argument_validation_without_gpu(libtt):
    from twotowermlretrieval_amd import _lib
    kmax, fmax = _header_define("TT_TOPK_LARGE_KMAX"), _header_define("TT_LEXICAL_FMAX")
    assert _topk(libtt, k=0) == _lib.TT_ERR_BAD_SHAPE and b"k=0" in libtt.tt_last_error()
    assert _topk(libtt, k=kmax + 1) == _lib.TT_ERR_UNSUPPORTED and b"k=" in libtt.tt_last_error()
    assert _topk(libtt, F=fmax + 1) == _lib.TT_ERR_UNSUPPORTED and b"TT_LEXICAL_FMAX" in libtt.tt_last_error()
    assert _topk(libtt, F=0) == _lib.TT_ERR_BAD_SHAPE
    assert _topk(libtt, indptr=None) == _lib.TT_ERR_BAD_SHAPE and b"null" in libtt.tt_last_error()
    need = libtt.tt_lexical_workspace_bytes(1, 100, 10)
    assert _topk(libtt, ws_bytes=need - 1) == _lib.TT_ERR_WORKSPACE
    assert _topk(libtt, ws=None) == _lib.TT_ERR_WORKSPACE
    assert _topk(libtt, out_idx=P + 4) == _lib.TT_ERR_BAD_SHAPE and b"aligned" in libtt.tt_last_error()
    assert _topk(libtt, out_val=P + 2) == _lib.TT_ERR_BAD_SHAPE
    assert _topk(libtt, indptr=P + 4) == _lib.TT_ERR_BAD_SHAPE
    assert _topk(libtt, N=-1) == _lib.TT_ERR_BAD_SHAPE
    assert _topk(libtt, N=2 ** 31 - 64, ws_bytes=1 << 40) == _lib.TT_ERR_UNSUPPORTED
    assert _topk(libtt, B=0, indptr=None, ws=None, ws_bytes=0) == _lib.TT_OK      # B = 0 does nothing
    # score_all: the shared checks
    assert libtt.tt_lexical_score_all_f32(None, P, P, 10, 257, P, P, P, 1, P, None) == _lib.TT_ERR_BAD_SHAPE
    assert libtt.tt_lexical_score_all_f32(P, P, P, 10, fmax + 1, P, P, P, 1, P, None) == _lib.TT_ERR_UNSUPPORTED
    assert libtt.tt_lexical_score_all_f32(P, P, P, 10, 257, P, P, P, 1, None, None) == _lib.TT_ERR_BAD_SHAPE
    assert libtt.tt_lexical_score_all_f32(P, P, P, 0, 257, P, P, P, 1, None, None) == _lib.TT_OK   # N = 0: nothing to write


def test_builder_sorts_sums_and_widens():
    sp = pytest.importorskip("scipy.sparse")
    from twotowermlretrieval_amd.lexical import csr_arrays, validate_csr
    # row 0: columns stored 5, 2, 5 (unsorted, one duplicate); row 1 empty; row 2: 1, 0
    data = np.array([1.0, 2.0, 0.5, 3.0, 4.0])
    indices = np.array([5, 2, 5, 1, 0], dtype=np.int32)
    indptr = np.array([0, 3, 3, 5], dtype=np.int32)
    m = sp.csr_matrix((data, indices, indptr), shape=(3, 7))
    m.has_sorted_indices = True                      # a stale flag, as fit_transform's result can carry: not to be trusted
    before = (m.data.copy(), m.indices.copy(), m.indptr.copy())
    ip, cols, vals, F = csr_arrays(m)
    assert F == 7 and ip.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.float32
    assert ip.tolist() == [0, 2, 2, 4] and cols.tolist() == [2, 5, 0, 1] and vals.tolist() == [2.0, 1.5, 4.0, 3.0]
    for a, b in zip(before, (m.data, m.indices, m.indptr)):
        assert np.array_equal(a, b)                  # built from a copy: the caller's matrix is untouched
    validate_csr(ip, cols, F, "t", True)
    ip2, cols2, vals2, _ = csr_arrays(m.tocsc())     # CSC in, the same CSR out
    assert ip2.tolist() == ip.tolist() and cols2.tolist() == cols.tolist() and vals2.tolist() == vals.tolist()
    with pytest.raises(TypeError):
        csr_arrays(np.zeros((2, 2)))


def test_validation_rejects_bad_matrices():
    from twotowermlretrieval_amd.lexical import validate_csr
    ip = np.array([0, 2, 3], dtype=np.int64)
    cols = np.array([0, 4, 1], dtype=np.int32)
    validate_csr(ip, cols, 5, "t", True)
    with pytest.raises(ValueError, match="column outside"):
        validate_csr(ip, cols, 4, "t", True)                                          # a column >= F
    with pytest.raises(ValueError, match="column outside"):
        validate_csr(ip, np.array([0, -1, 1], dtype=np.int32), 5, "t", True)
    with pytest.raises(ValueError, match="decreases"):
        validate_csr(np.array([0, 3, 2, 3], dtype=np.int64), cols, 5, "t", True)     # a decreasing indptr
    with pytest.raises(ValueError, match=r"indptr\[0\]"):
        validate_csr(np.array([1, 2, 3], dtype=np.int64), cols, 5, "t", True)
    with pytest.raises(ValueError, match="entries are stored"):
        validate_csr(np.array([0, 2, 4], dtype=np.int64), cols, 5, "t", True)
    with pytest.raises(ValueError, match="ascending"):
        validate_csr(ip, np.array([4, 0, 1], dtype=np.int32), 5, "t", True)
    validate_csr(ip, np.array([0, 4, 0], dtype=np.int32), 5, "t", True)               # a new row may start lower


def test_product_refuses_cpu_tensors():
    import twotowermlretrieval_amd as tt
    ip, cols, vals = torch.tensor([0, 1]), torch.tensor([0], dtype=torch.int32), torch.tensor([1.0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.LexicalIndex((ip, cols, vals, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.lexical_score_topk((ip, cols, vals), 4, (ip, cols, vals), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.lexical_score_all((ip, cols, vals), 4, (ip, cols, vals))
    sp = pytest.importorskip("scipy.sparse")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tt.LexicalIndex(sp.csr_matrix(np.eye(3, dtype=np.float32)), device="cpu")
    with pytest.raises(ValueError, match="lexical must be"):
        tt.HybridSearcher(None, ["a"], index=object(), lexical="cuda")


def test_reference_helper_on_a_hand_case():
    """lexical_ref against values worked out by hand: order of the adds, the column guard, ties by index."""
    indptr = np.array([0, 3, 3, 5], dtype=np.int64)
    cols = np.array([0, 2, 9, 1, 2], dtype=np.int32)              # column 9 >= F = 4 contributes nothing
    vals = np.array([0.5, 0.25, 7.0, 1.0, 0.25], dtype=np.float32)
    q = ref.dense_query([2, 0, 11], [2.0, 1.0, 5.0], 4)           # the query's column 11 is dropped as well
    assert q.tolist() == [1.0, 0.0, 2.0, 0.0]
    s32 = ref.ref_scores32(indptr, cols, vals, q)
    assert s32.dtype == np.float32 and s32.tolist() == [1.0, 0.0, 0.5]
    assert ref.ref_scores64(indptr, cols, vals, q).tolist() == [1.0, 0.0, 0.5]
    v, i = ref.ref_topk(np.array([0.5, 1.0, 0.5, np.nan, 1.0], dtype=np.float32), 4)
    assert i.tolist() == [1, 4, 0, 2] and v.tolist() == [1.0, 1.0, 0.5, 0.5]
    v, i = ref.ref_topk(np.array([0.5, 1.0, 0.5], dtype=np.float32), 3, keep=[True, False, True], min_score=0.5, idx_offset=10)
    assert i.tolist() == [10, 12, -1] and v.tolist() == [0.5, 0.5, -np.inf]
    # the chain is sequential: (1 + 2^-24) + 2^-24 in float32 stays 1, a pairwise sum would not
    e = np.float32(2.0 ** -24)
    s = ref.ref_scores32(np.array([0, 3]), np.array([0, 1, 2]), np.array([1.0, e, e], dtype=np.float32), np.ones(3, np.float32))
    assert s[0] == np.float32(1.0)


def _zipf_docs(rng, n_docs, vocab, lo=5, hi=60):
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    return [" ".join(f"w{t}" for t in rng.choice(vocab, size=int(rng.integers(lo, hi)), p=p)) for _ in range(n_docs)]


def test_f32_chain_is_within_the_bound_of_sklearn_cosine():
    """|ref_scores32 - cosine_similarity| <= (m + 3) * 2^-24 for a query of m terms: the f32 rounding of a value, of a query
    weight, of a product and of each of the m - 1 adds contributes at most 2^-24 of a partial sum, and the partial sums of
    unit-norm non-negative rows are <= 1 + eps."""
    pytest.importorskip("sklearn")
    from sklearn.feature_extraction.text import TfidfVectorizer
    from sklearn.metrics.pairwise import cosine_similarity
    from twotowermlretrieval_amd.lexical import csr_arrays
    rng = np.random.default_rng(7)
    docs = _zipf_docs(rng, 3000, 2000)
    tfidf = TfidfVectorizer(max_features=20000)
    mat = tfidf.fit_transform(docs)
    indptr, cols, vals, F = csr_arrays(mat)
    queries = docs[:8] + _zipf_docs(rng, 25, 2000, 1, 12)
    worst = 0.0
    for text in queries:
        qm = tfidf.transform([text])
        _, qc, qv, _ = csr_arrays(qm)
        m = qc.size
        want = cosine_similarity(qm, mat)[0]
        got = ref.ref_scores32(indptr, cols, vals, ref.dense_query(qc, qv, F))
        bound = (m + 3) * 2.0 ** -24
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst = max(worst, err / bound)
        assert err <= bound, (text[:40], m, err, bound)
    print(f"worst |f32 chain - sklearn cosine| / bound = {worst:.3f}")
