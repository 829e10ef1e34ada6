"""The planted-row layout of tests/big_corpus.py, checked without a GPU: positions on both sides of every width boundary, the
shares beyond them, the duplicate pairs, the mask's removals, and the margin between the planted scores the GPU cases rely on
and the bound build_corpus() enforces on the background (BG_NORM_MAX).  Prints the figures big_corpus.py's docstring quotes."""
import numpy as np
import pytest

import big_corpus as bc


@pytest.fixture(scope="module", params=[256, 512])
def layout(request):
    return bc.Layout(request.param)


def test_positions(layout):
    n, u, pos, group = layout.n, layout.unit, layout.pos, layout.group
    assert n == {256: 2 ** 24 + 2 ** 16 + 77, 512: 2 ** 23 + 2 ** 15 + 77}[layout.d] and n % 32 and n < 2 ** 31 - 64
    assert u * layout.d * 4 == 2 ** 32 and 4 * u * layout.d == 2 ** 32 and n * layout.d > 2 ** 32
    assert (np.diff(pos) > 0).all() and pos[0] == 0 and pos[-1] == n - 1
    for j in range(1, 5):
        assert np.isin([u * j - 1, u * j, u * j + 1], pos).all()
    full = (pos >= layout.last_full) & (pos < layout.last_full + 32)
    assert layout.last_full + 32 <= n < layout.last_full + 64 and full.sum() >= 3
    assert (group == 0).sum() == bc.GROUP0 and all((group == g).sum() == bc.GROUP_N for g in range(1, bc.G))
    for g in range(bc.G):
        rows = pos[group == g]
        assert 2 * (rows > 4 * u).sum() >= len(rows) and 4 * ((rows >= 2 * u) & (rows <= 4 * u)).sum() >= len(rows)
        assert (layout.band(rows) == np.arange(5)[:, None]).any(1).all()        # every group has rows in every band
    assert len(layout.dups) == 8
    for low, high in layout.dups:
        assert pos[low] < u and pos[high] > 4 * u and group[low] == group[high] and np.array_equal(layout.rows[low], layout.rows[high])
    assert np.abs(np.linalg.norm(layout.rows.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_mask(layout):
    cols, bg = layout.removals()
    keep = layout.keep_bool(cols, bg)
    assert not np.isin(bg, layout.pos).any() and len(bg) > 90_000 and (bg > 4 * layout.unit).any()
    assert not keep[layout.pos[cols]].any() and keep[np.delete(layout.pos, cols)].all() and (~keep).sum() == len(cols) + len(bg)
    band = layout.band(layout.pos[cols])
    assert all((band == b).sum() >= 10 for b in range(5))
    assert (layout.group == 0).sum() - (layout.group[cols] == 0).sum() >= 100 + 300
    words = bc.pack_bits(keep)
    assert len(words) == (layout.n + 31) // 32 and words[-1] >> (layout.n % 32) == 0
    for r in (0, 31, 32, int(layout.pos[cols][-1]), layout.n - 1):
        assert bool(words[r >> 5] >> (r & 31) & 1) == bool(keep[r])


def test_planted_scores_clear_the_background_bound(layout, oracle):
    """Same-group scores against the largest floor the background bound allows (1.05 x 0.6); other-group scores below it, so
    that a case's k-th score is a same-group row's wherever its validity assertion holds."""
    floor = bc.FLOOR_FACTOR * bc.BG_NORM_MAX
    Q, groups = layout.small_queries()
    Q0 = layout.group0_queries()
    for name, P in (("fp32", layout.rows), ("bf16", bc.to_bf16(layout.rows))):
        S, S0 = oracle.score_all(Q, P), oracle.score_all(Q0, P)
        same = layout.group[None, :] == groups[:, None]
        lo = min(float(S[same].min()), float(S0[:, layout.group == 0].min()))
        other = max(float(S[~same].max()), float(S0[:, layout.group != 0].max()))
        print(f"d = {layout.d} {name}: smallest same-group score {lo:.4f}, largest other-group score {other:.4f}, floor <= {floor:.3f}")
        assert lo > floor > other
        cols, _ = layout.removals()
        ref = bc.Reference(oracle, layout, name == "bf16", bc.BG_NORM_MAX)
        ref.topk(S, 64)
        ref.topk(S, 64, removed=cols)
        ref.topk(S0, 1000)
        ref.topk(S0, 100, removed=cols)
