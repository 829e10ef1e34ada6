"""Every *_workspace_bytes and *_offset query of the search family at corpus sizes up to the largest N an entry accepts
(2^31 - 65 rows): the planners run in host arithmetic, and an intermediate that wrapped at 32 bits would hand a search a
workspace that is too small for exactly the corpora the kernels' 64-bit row addresses are there for.  No GPU, no compute call.

For each query, over B in {1, 64, 65, 1024}, the k and d its entry allows and both dtypes:
  - the size is positive and non-decreasing in N over {2^22, 2^24, 10^8, 2^31 - 65};
  - in particular the value at 2^31 - 65 is at least the value at 10^8 (a wrapped product would make it smaller);
  - every offset a query reports lies inside the workspace of the same shape with room for the words include/tt.h says
    it holds (int32 words: 4-byte aligned), or is (size_t)-1 where the header says the shape has none."""
import ctypes
import itertools
import math

import pytest

from test_abi_cpu import libtt  # noqa: F401  (the fixture builds the library when it is missing)

NS = (2 ** 22, 2 ** 24, 10 ** 8, 2 ** 31 - 65)
BS = (1, 64, 65, 1024)
NONE = ctypes.c_size_t(-1).value
K_SMALL = (10, 64)
K_LARGE = (10, 64, 65, 1024)
D_OF = {0: (256, 512), 1: (256,)}      # bf16 = 0 / 1 -> the widths at which both the exact f32 and the exact bf16 entries exist


def _sizes():
    """(name, function of (lib, B, N), tuple naming the shape) for every workspace query and shape of the grid."""
    out = []
    for bf16 in (0, 1):
        small = "tt_score_topk_bf16_workspace_bytes" if bf16 else "tt_score_topk_workspace_bytes"
        screened = "tt_score_topk_screened_bf16_workspace_bytes" if bf16 else "tt_score_topk_screened_workspace_bytes"
        for d in D_OF[bf16]:
            for k in K_SMALL:
                out.append((small, lambda L, B, N, n=small, d=d, k=k: getattr(L, n)(B, N, d, k), (d, k)))
            for k in K_LARGE:
                for name in ("tt_score_topk_large_workspace_bytes", "tt_score_topk_masked_workspace_bytes"):
                    out.append((name, lambda L, B, N, n=name, d=d, k=k, t=bf16: getattr(L, n)(B, N, d, k, t), (d, k, bf16)))
            out.append(("tt_score_count_workspace_bytes",
                        lambda L, B, N, d=d, t=bf16: L.tt_score_count_workspace_bytes(B, N, d, t), (d, bf16)))
        for k in K_SMALL:                 # the screen: d = 256, k <= 64
            out.append((screened, lambda L, B, N, n=screened, k=k: getattr(L, n)(B, N, 256, k), (256, k)))
            out.append(("tt_score_topk_screened_masked_workspace_bytes",
                        lambda L, B, N, k=k, t=bf16: L.tt_score_topk_screened_masked_workspace_bytes(B, N, 256, k, t), (256, k, bf16)))
    return out


SIZES = _sizes()


@pytest.mark.parametrize("case", range(len(SIZES)), ids=[f"{n}{s}" for n, _, s in SIZES])
def test_sizes_grow_with_the_corpus(libtt, case):  # noqa: F811
    name, size, shape = SIZES[case]
    for B in BS:
        got = [size(libtt, B, N) for N in NS]
        print(name, shape, "B", B, got)
        assert all(0 < g < 2 ** 48 for g in got), (name, shape, B, got)       # (neither refused nor a wrapped negative)
        assert all(a <= b for a, b in zip(got, got[1:])), (name, shape, B, got)
        assert got[3] >= got[2], (name, shape, B, got)


def _inside(off, words, total, what):
    assert off != NONE, what
    assert off % 4 == 0 and 0 < off and off + 4 * words <= total, (what, off, words, total)


def test_exact_diagnostic_offsets(libtt):  # noqa: F811
    """The pace time-out count (one int32) and the redo flags (one int32 per 32-query tile) of the k <= 64 exact search: where the
    shape has them they sit inside both dtypes' workspaces (one layout above 16 queries); a shape the header excludes says so at
    every N alike."""
    pace, redo = libtt.tt_score_topk_pace_timeouts_offset, libtt.tt_score_topk_redo_flags_offset
    sizes = (libtt.tt_score_topk_workspace_bytes, libtt.tt_score_topk_bf16_workspace_bytes)
    seen = 0
    for B, N, k, d in itertools.product(BS, NS, K_SMALL, (256, 512)):
        totals = [q(B, N, d, k) for q in (sizes if d == 256 and B > 16 else sizes[:1])]
        po, ro = pace(B, N, d, k), redo(B, N, d, k)
        if B < 65 or d == 512:           # fewer than three 32-query tiles, or 16-query tiles: never paced, no shared pool
            assert po == NONE and ro == NONE, (B, N, k, d)
            continue
        for total in totals:
            _inside(po, 1, total, ("pace", B, N, k, d))
            _inside(ro, (B + 31) // 32, total, ("redo", B, N, k, d))
        seen += 1
    assert seen == 2 * len(NS) * len(K_SMALL)


def test_large_tier_offset(libtt):  # noqa: F811
    """One int32 per query inside the large (and therefore the masked) call's workspace, at every k the entry takes."""
    for bf16 in (0, 1):
        for B, N, k, d in itertools.product(BS, NS, K_LARGE, D_OF[bf16]):
            off = libtt.tt_score_topk_large_tier_offset(B, N, d, k, bf16)
            total = libtt.tt_score_topk_large_workspace_bytes(B, N, d, k, bf16)
            _inside(off, B, total, ("tier", B, N, k, d, bf16))
            assert libtt.tt_score_topk_masked_workspace_bytes(B, N, d, k, bf16) == total


def test_screened_stats_offset(libtt):  # noqa: F811
    """int32 [B][2] inside the screen's own part of all four screened workspaces (the query takes no dtype: one offset)."""
    for B, N, k in itertools.product(BS, NS, K_SMALL):
        off = libtt.tt_score_topk_screened_stats_offset(B, N, 256, k)
        for total in (libtt.tt_score_topk_screened_workspace_bytes(B, N, 256, k),
                      libtt.tt_score_topk_screened_bf16_workspace_bytes(B, N, 256, k),
                      libtt.tt_score_topk_screened_masked_workspace_bytes(B, N, 256, k, 0),
                      libtt.tt_score_topk_screened_masked_workspace_bytes(B, N, 256, k, 1)):
            _inside(off, 2 * B, total, ("stats", B, N, k))


# ---- lexical search and the in-batch loss --------------------------------------------------------------------------------------
LEX_BS = (1, 64, 65, 1024, 65535)
LEX_CHUNK = 4096


def test_lexical_workspace_grows_with_the_corpus(libtt):  # noqa: F811
    """tt_lexical_workspace_bytes(B, N, k): one float and one int64 per entry of every chunk's partial list at least (12 B k
    ceil(N / 4096) bytes), positive, non-decreasing in N, not wrapped; 0 for the shapes the call refuses.
    "Not wrapped" is below 2^48 wherever the lower bound itself is (at B = 65535, k = 1024, N = 2^31 - 65 the lists alone are
    12 x 65535 x 1024 x 524288 = 4.2e14 bytes > 2^48 = 2.8e14: no size can satisfy both), and everywhere at most what the plan
    can need: above 64 chunks the lists are padded to groups of per = ceil(sqrt(chunks)) -- fewer than chunks + per lists --
    and the first merge writes one list per group, at most per + 1: 12 B k (chunks + 2 per + 1) bytes plus alignment."""
    size = libtt.tt_lexical_workspace_bytes
    assert libtt.tt_lexical_chunk_docs() == LEX_CHUNK
    for B, k in itertools.product(LEX_BS, K_LARGE):
        got = [size(B, N, k) for N in NS]
        print("tt_lexical_workspace_bytes", "B", B, "k", k, got)
        assert all(a <= b for a, b in zip(got, got[1:])), (B, k, got)
        for N, g in zip(NS, got):
            chunks = -(-N // LEX_CHUNK)
            per = math.isqrt(chunks - 1) + 1
            least = 12 * B * k * chunks
            assert 0 < least <= g <= 12 * B * k * (chunks + 2 * per + 1) + 4096, (B, N, k, g)
            assert g < 2 ** 48 or least >= 2 ** 48, (B, N, k, g)
        assert size(B, 2 ** 31 - 64, k) == 0 and size(B, 2 ** 31 - 65, k) == got[3]
    for B in LEX_BS:
        assert size(B, NS[1], 0) == 0 and size(B, NS[1], 1025) == 0 and size(B, NS[1], 1024) > 0
    for k in K_LARGE:
        assert size(0, NS[1], k) == 0


def test_in_batch_loss_workspace_grows_with_the_batch(libtt):  # noqa: F811
    """tt_in_batch_loss_workspace_bytes(B, H): at least the two images, 4 (Bq + Dp) Hp bytes with Hp = H up to a multiple of 32
    and Bq / Dp = B / 2 B up to multiples of 128 (ib_plan), positive, non-decreasing in B and in H; 0 beyond B = 2^24 or
    H = 512."""
    size = libtt.tt_in_batch_loss_workspace_bytes
    BS_IB, HS = (1, 512, 1025, 65536, 2 ** 24), (1, 20, 512)
    got = {(B, H): size(B, H) for B in BS_IB for H in HS}
    print("tt_in_batch_loss_workspace_bytes", got)
    for (B, H), g in got.items():
        Hp, Bq, Dp = -(-H // 32) * 32, -(-B // 128) * 128, -(-2 * B // 128) * 128
        assert 4 * (Bq + Dp) * Hp <= g < 2 ** 48, (B, H, g)
    for H in HS:
        col = [got[B, H] for B in BS_IB]
        assert all(a <= b for a, b in zip(col, col[1:])), (H, col)
    for B in BS_IB:
        row = [got[B, H] for H in HS]
        assert all(a <= b for a, b in zip(row, row[1:])), (B, row)
    assert size(2 ** 24 + 1, 20) == 0 and size(512, 513) == 0 and size(0, 20) == 0 and size(512, 0) == 0
