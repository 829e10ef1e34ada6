"""The encoder forward, its backward, the weight-gradient products and the table paths where their 64-bit addresses pass
2^32 bytes, 2^31 and 2^32 elements -- x, gates, gi, dgi, dghn, dx at tok * ld (csrc/encoder.h: EncLayout), the projected table
at id * 3H, the trainable table and its gradient at id * E -- and on both sides of the two limits that are 32-bit on purpose
(wgrad16's B byte offsets: tt_wgrad16_supported).  tests/encoder_big.py says how the reference stays cheap: sampled rows in
float64 on a compact table, output cotangents that are zero off the sampled rows, and for inference every row bit-equal to the
same ids in calls of 8 192 rows.  Tolerances are conftest.FWD_ATOL and GRAD_TOL (floor 1e-6), nothing else.

One big workspace is alive at a time; every test frees its tensors and empties the allocator's cache on the way out.

Not checked here: the inter-layer dropout mask past 2^32 padded elements (case 7 runs p = 0: the float64 reference has no such
mask and the C oracle's mask takes no row offset, so sampled rows cannot keep their padded indices), and backward passes of
rows longer than 128 tokens."""
import functools

import numpy as np
import pytest
import torch

import encoder_big as eb
import synth

pytestmark = pytest.mark.gpu

CHUNK = 8192
SPLIT_B = 512                                               # a batch of the column-split recurrence (gru16x4: B <= 1024)


@pytest.fixture(autouse=True)
def _free_on_exit():
    yield
    eb.release()


def _plan(name, B, T, by_width, seed, must_cross):
    """(lens, tok_off, boundaries, sampled rows) of a B x T batch of varied lengths; must_cross: [(buffer, boundary label)]."""
    lens = eb.varied_lens(B, T)
    tok_off = eb.tok_offsets(lens)
    bounds = eb.boundaries(tok_off, by_width)
    rows = eb.sample_rows(B, tok_off, bounds, seed)
    eb.describe(name, B, T, tok_off, bounds, rows)
    for buf, label in must_cross:
        assert eb.crossed(bounds, buf, label), (buf, label, int(tok_off[-1]))
    return lens, tok_off, bounds, rows


def _chunked(enc, ids):
    return torch.cat([enc(ids[lo:lo + CHUNK]) for lo in range(0, ids.shape[0], CHUNK)], 0)


# ---- cases 1 and 2: inference, the projecting call ----------------------------------------------------------------------------
INFER = {
    # gru16 with two row tiles; gi [tokens][768] crosses all three boundaries (workspace 17.8 GB)
    "one_layer_5m7": dict(B=82944, T=70, layers=1, bi=False, arith="split16",
                          cross=[("gi", "2^32 bytes"), ("gi", "2^31 elements"), ("gi", "2^32 elements")]),
    # the fp32 recurrence (gru_seq_kernel) over the first half of the same batch
    "one_layer_2m9_f32": dict(B=41472, T=70, layers=1, bi=False, arith="f32", cross=[("gi", "2^31 elements")]),
    # x[1] [tokens][512] feeds layer 1's K1 through the wide gemm_rows16 form; gi of both layers crosses 2^31 elements
    # (B a multiple of 8 192: below 2 048 rows the Linear(2H, H) head is one kernel instead of two GEMMs, other bits)
    "two_layers_bi_2m8": dict(B=40960, T=70, layers=2, bi=True, arith="split16",
                              cross=[("gi", "2^31 elements"), ("x", "2^32 bytes")]),
}


@pytest.mark.parametrize("cid", list(INFER))
def test_inference_sampled_rows_vs_float64_and_every_row_vs_calls_of_8192_rows(cid):
    c = INFER[cid]
    B, T, layers, bi, E, H, V = c["B"], c["T"], c["layers"], c["bi"], 300, 256, 30000
    lens, tok_off, bounds, rows = _plan(cid, B, T, eb.per_token_buffers("GRU", E, H, layers, bi, False), 11, c["cross"])
    ws = eb.workspace_bytes("GRU", B, T, E, H, layers, bi, 0)
    eb.require_memory(cid, workspace=ws, ids=B * T * 8, table=V * E * 4, outputs=2 * B * H * 4)
    table = eb.device_table(V, E, 21)
    ids = eb.device_ids(lens, T, V, 22)
    enc, sd = eb.make_encoder("GRU", E, H, layers, bi, 23, table, arith=c["arith"])
    enc.eval()
    assert not bi or B % CHUNK == 0                        # every call of a bidirectional model on the two-GEMM head (B >= 2048)
    rows_dev = torch.from_numpy(rows).cuda()
    with torch.no_grad():
        y = enc(ids)
        torch.cuda.synchronize()
        _, want, _, _ = eb.reference("GRU", ids[rows_dev].cpu().numpy(), table, sd, E, H, layers, bi)
        eb.fwd_check(cid, y[rows_dev].cpu().numpy(), want)
        parts = _chunked(enc, ids)
    differ = int((parts != y).any(dim=1).sum())
    print(f"[{cid}] rows that differ from the {CHUNK}-row calls: {differ} of {B}")
    assert torch.equal(parts, y)


# ---- case 3: the column-split recurrence on long rows ---------------------------------------------------------------------------
def test_column_split_recurrence_long_rows_vs_oracle_and_vs_one_workgroup(oracle):
    """gru16x4 (B <= 1024): 1 024 rows of about 2 816 tokens, gi past 2^31 elements.  Four rows -- first, last, the two at the
    boundary -- against the C oracle's forward; every row bit-equal to the one-workgroup recurrence (gru16), as the header of
    csrc/gru16x4.hip promises.  The status word is read here: a call that gave the hand-off up would be redone on gru16 by
    RNNEncoder.forward and compare gru16 with itself."""
    name, B, T, E, H, V = "split_1024x2816", 1024, 2816, 300, 256, 30000
    lens, tok_off, bounds, _ = _plan(name, B, T, eb.per_token_buffers("GRU", E, H, 1, False, False), 12, [("gi", "2^31 elements")])
    top = [bd for bd in bounds if bd["boundary"] == "2^31 elements"][0]["row"]
    rows = np.array([0, top, top + 1, B - 1], dtype=np.int64)
    print(f"[{name}] rows against the oracle: {rows.tolist()}")
    ws = eb.workspace_bytes("GRU", B, T, E, H, 1, False, 0)
    eb.require_memory(name, workspace=ws, ids=B * T * 8, table=V * E * 4)
    table = eb.device_table(V, E, 31)
    ids = eb.device_ids(lens, T, V, 32)
    enc, sd = eb.make_encoder("GRU", E, H, 1, False, 33, table)
    enc.eval()
    assert enc.split_workgroups(B) > 0                     # this shape takes the column-split kernels on this device
    enc.check_inputs = False
    with torch.no_grad():
        y, _, status = enc._run_forward(ids, train=False)
        assert int(status.item()) == 0, "the column-split recurrence reported a status: nothing was compared"
        enc.one_workgroup = True
        y1, _, status1 = enc._run_forward(ids, train=False)
        assert int(status1.item()) == 0
    differ = int((y1 != y).any(dim=1).sum())
    print(f"[{name}] rows that differ between gru16x4 and gru16: {differ} of {B}")
    assert torch.equal(y, y1)
    rows_dev = torch.from_numpy(rows).cuda()
    want = oracle.encoder_forward(ids[rows_dev].cpu().numpy(), table.cpu().numpy(), synth.weight_quads(sd), H)
    eb.fwd_check(name, y[rows_dev].cpu().numpy(), want, what="_vs_oracle")


# ---- case 4: the projected table -------------------------------------------------------------------------------------------------
def test_projected_table_past_2_31_and_2_32_elements():
    """P [V][768] of 5.7 M vocabulary rows (17.5 GB), gathered at id * 768: ids from the two ends of the table and from both
    sides of the rows where P passes 2^31 and 2^32 elements.  projected_table = True (the automatic mode stops at 8 GB).
    The gather is written three times -- gru16x4, gru16 with one row tile and with two -- so the batch is run at the sizes that
    reach each; every call returns the bits of the call that projects its own tokens."""
    from twotowermlretrieval_amd import _lib
    name, V, E, H, B, T = "projected_5m7", 5_700_000, 64, 256, 16384, 64
    H3 = 3 * H
    r31, r32 = -(-2 ** 31 // H3), -(-2 ** 32 // H3)        # the first row that starts at or past the boundary
    assert r32 + 100 < V - 100 and (r31 - 1) * H3 < 2 ** 31 <= r31 * H3 and (r32 - 1) * H3 < 2 ** 32 <= r32 * H3
    zones = [(1, 100), (r31 - 100, r31), (r31, r31 + 100), (r32 - 100, r32), (r32, r32 + 100), (V - 100, V)]
    print(f"\n[{name}] P [{V}][{H3}]: 2^31 elements at row {r31}, 2^32 elements at row {r32}; id zones {zones}")
    pbytes = int(_lib.lib().tt_encoder_projected_bytes(V, E, H, 0, 0))
    assert pbytes >= V * H3 * 4 > 2 ** 32 * 4
    ws = eb.workspace_bytes("GRU", B, T, E, H, 1, False, 0)
    eb.require_memory(name, projected=pbytes, table=V * E * 4, workspace=ws)
    lens = eb.varied_lens(B, T)
    table = eb.device_table(V, E, 41)
    ids = eb.device_ids(lens, T, V, 42, zones=zones)
    for lo, hi in zones:
        n = int(((ids >= lo) & (ids < hi)).sum())
        print(f"[{name}] ids in [{lo}, {hi}): {n}")
        assert n >= 64
    rows = np.unique(np.concatenate([[0, B - 1], np.random.RandomState(43).choice(B, eb.MAX_ROWS - 2, replace=False)]))[:eb.MAX_ROWS]
    rows_dev = torch.from_numpy(rows).cuda()
    ids_rows = ids[rows_dev].cpu().numpy()
    assert all(((ids_rows >= lo) & (ids_rows < hi)).sum() >= 16 for lo, hi in zones)
    enc, sd = eb.make_encoder("GRU", E, H, 1, False, 44, table)
    enc.eval()
    enc.check_inputs = False
    assert enc.split_workgroups(SPLIT_B) > 0 and enc.split_workgroups(4096) == 0

    def call(n, one_workgroup):
        enc.one_workgroup = one_workgroup
        y, _, status = enc._run_forward(ids[:n], train=False)
        assert int(status.item()) == 0                      # (a split recurrence that gave up would be no gather of gru16x4)
        return y

    # each form of the gather has its own address: gru16x4 (B <= 1024), gru16 with one row tile and with two (B >= 8192)
    forms = [("gru16x4", SPLIT_B, False), ("gru16, one row tile, 512 rows", SPLIT_B, True), ("gru16, one row tile", 4096, False),
             ("gru16, two row tiles", B, False)]
    with torch.no_grad():
        for what, n, one in forms:
            for lo, hi in zones:
                assert int(((ids[:n] >= lo) & (ids[:n] < hi)).sum()) >= 64
            enc.projected_table = False
            plain = call(n, one).clone()
            enc.projected_table = True
            proj = call(n, one)
            assert ids.device in enc._proj and enc._proj[ids.device][1].numel() == pbytes
            differ = int((proj != plain).any(dim=1).sum())
            print(f"[{name}] {what}: rows that differ between the projected and the projecting call: {differ} of {n}")
            assert torch.equal(proj, plain), what
    _, want, _, _ = eb.reference("GRU", ids_rows, table, sd, E, H, 1, False)
    eb.fwd_check(name, proj[rows_dev].cpu().numpy(), want)
    enc.invalidate_prepared()


# ---- cases 5, 6, 7: training --------------------------------------------------------------------------------------------------
TRAIN = {
    # gates / gi / dgi / dghn past 2^31 elements; dW_hh on wgrad16 with B byte offsets past 2^31 ((MT + 1) 256 < 2^30)
    "gru256_2m9": dict(cell="GRU", B=41472, T=70, E=300, H=256, layers=1, bi=False, arith="split16",
                       cross=[(b, "2^31 elements") for b in ("gates", "gi", "dgi", "dghn")]),
    # the same buffers past 2^32 elements; (MT + 1) 256 >= 2^30: dW_hh leaves wgrad16 for the tiled product
    "gru256_5m7": dict(cell="GRU", B=82944, T=70, E=300, H=256, layers=1, bi=False, arith="split16",
                       cross=[(b, "2^32 elements") for b in ("gates", "gi", "dgi", "dghn")]),
    # the same batch with arith="f32": gru_seq_kernel<8> / gru_bwd_seq_kernel<8> and the column-sum passes (colsum_kernel: the
    # bias gradients and operand maxima that the f16-split recurrence computes itself) over dgi / dghn past 2^32 elements
    "gru256_5m7_f32": dict(cell="GRU", B=82944, T=70, E=300, H=256, layers=1, bi=False, arith="f32",
                           cross=[(b, "2^32 elements") for b in ("gates", "gi", "dgi", "dghn")]),
    # the fp32 kernels gru_seq_kernel<16> / gru_bwd_seq_kernel<16>: 1 536 floats per token in gi / dgi
    "gru512_1m45": dict(cell="GRU", B=20800, T=70, E=64, H=512, layers=1, bi=False, arith="split16",
                        cross=[("gi", "2^31 elements"), ("dgi", "2^31 elements"), ("gates", "2^31 elements")]),
    # LSTM: gates and dgi are 4H wide; cseq has the row MT
    "lstm256_2m2": dict(cell="LSTM", B=31744, T=70, E=64, H=256, layers=1, bi=False, arith="split16",
                        cross=[("gates", "2^31 elements"), ("dgi", "2^31 elements"), ("gi", "2^31 elements")]),
    # two layers, both directions (p = 0: module docstring): x / dx [tokens][512] past 2^31 elements
    "gru256_2l_bi_4m2": dict(cell="GRU", B=61440, T=70, E=300, H=256, layers=2, bi=True, arith="split16",
                             cross=[("x", "2^31 elements"), ("dx", "2^31 elements"), ("gates", "2^32 elements")]),
}


def _train_and_check(name, c, lens, rows, V=30000, zones=None, trainable=False, table=None, seed=50):
    """One training step of the whole batch with the cotangent on `rows` alone; the rows' outputs and every gradient against
    float64 over those rows.  Returns (encoder, ids, used ids, float64 table gradient at the used ids, gradients as numpy)."""
    cell, B, T, E, H, layers, bi = c["cell"], c["B"], c["T"], c["E"], c["H"], c["layers"], c["bi"]
    if table is None:
        table = eb.device_table(V, E, seed + 1)
    ids = eb.device_ids(lens, T, V, seed + 2, zones=zones)
    enc, sd = eb.make_encoder(cell, E, H, layers, bi, seed + 3, table, trainable=trainable, arith=c.get("arith", "split16"))
    enc.train()
    rows_dev = torch.from_numpy(rows).cuda()
    d_out, d_rows = eb.cotangent(B, H, rows, seed + 4)
    used, want, wg, wt = eb.reference(cell, ids[rows_dev].cpu().numpy(), table, sd, E, H, layers, bi, d_out=d_rows, table_grad=trainable)
    y = enc(ids)
    eb.fwd_check(name, y.detach()[rows_dev].cpu().numpy(), want)
    assert bool(torch.isfinite(y).all())
    y.backward(d_out)
    torch.cuda.synchronize()
    del y, d_out
    got = eb.check_parameter_grads(name, enc, wg)
    return enc, ids, used, wt, got


@pytest.mark.parametrize("cid", list(TRAIN))
def test_training_step_outputs_and_every_gradient_vs_float64(cid):
    c = TRAIN[cid]
    cell, B, T, E, H, layers, bi = c["cell"], c["B"], c["T"], c["E"], c["H"], c["layers"], c["bi"]
    lens, tok_off, bounds, rows = _plan(cid, B, T, eb.per_token_buffers(cell, E, H, layers, bi, True), 13, c["cross"])
    print(f"[{cid}] dW_hh B operand: (MT + 1) x ndir H = {(B * T + 1) * (2 if bi else 1) * H} elements (wgrad16 below 2^30 = {2 ** 30})")
    ws = eb.workspace_bytes(cell, B, T, E, H, layers, bi, 1)
    eb.require_memory(cid, workspace=ws, ids=B * T * 8, table=30000 * E * 4, outputs=2 * B * H * 4)
    _train_and_check(cid, c, lens, rows)


# ---- case 8: wgrad16's limits, layer 0 (B rows through ids) -------------------------------------------------------------------
EDGE = 50                                                   # ids come from [1, EDGE) and [V - EDGE, V)
LAYER0 = [(4_194_303, 256), (4_194_304, 256), (16_777_215, 64), (16_777_216, 64)]
TINY = dict(cell="GRU", B=9, T=11, H=256, layers=1, bi=False)


def _edge_table(V, E, seed, fill_seed):
    """A [V, E] table on the device whose first and last EDGE rows are the same host rows whatever V is."""
    table = eb.device_table(V, E, fill_seed)
    ends = (np.random.RandomState(seed).standard_normal((2 * EDGE, E)) * 0.3).astype(np.float32)
    table[:EDGE] = torch.from_numpy(ends[:EDGE]).cuda()
    table[V - EDGE:] = torch.from_numpy(ends[EDGE:]).cuda()
    return table


@functools.lru_cache(maxsize=None)
def _layer0(V, E):
    """The tiny batch over a V x E frozen table: every gradient checked against float64, returned as numpy.  The two sizes of a
    pair see the same problem: the same rows at the two ends of the table, the same ids counted from the ends."""
    name = f"layer0_V{V}_E{E}"
    c = dict(TINY, E=E)
    B, T, H = c["B"], c["T"], c["H"]
    print(f"\n[{name}] V E = {V * E} = 2^30 {V * E - 2 ** 30:+d}; last row ends {2 ** 32 - V * E * 4} bytes below 2^32; "
          f"{'wgrad16' if V < 2 ** 24 and V * E < 2 ** 30 else 'the tiled product'} by tt_wgrad16_supported")
    ws = eb.workspace_bytes("GRU", B, T, E, H, 1, False, 1)
    eb.require_memory(name, table=V * E * 4, workspace=ws)
    lens = eb.varied_lens(B, T)
    rows = np.arange(B, dtype=np.int64)
    table = _edge_table(V, E, 61, 62)
    # (device_ids draws the zone, then the offset inside it: with zones of one width the draws do not depend on V)
    _, ids, used, _, got = _train_and_check(name, c, lens, rows, V=V, zones=[(1, EDGE), (V - EDGE + 1, V)], table=table, seed=60)
    assert (used[1:] < EDGE).sum() >= 10 and (used >= V - EDGE).sum() >= 10 and int(ids.max()) >= V - EDGE
    del table, ids
    eb.release()
    return got


@pytest.mark.parametrize("V,E", LAYER0)
def test_wgrad16_limit_table_rows_through_ids_vs_float64(V, E):
    _layer0(V, E)


@pytest.mark.parametrize("pair", [(LAYER0[0], LAYER0[1]), (LAYER0[2], LAYER0[3])], ids=["E256", "E64"])
def test_wgrad16_limit_both_sides_agree(pair):
    below, at = _layer0(*pair[0]), _layer0(*pair[1])
    assert set(below) == set(at)
    for key in sorted(below):
        eb.grad_check(f"pair_E{pair[0][1]}", key + " (wgrad16 vs tiled)", below[key], at[key].astype(np.float64))


# ---- case 9: wgrad16's limit, dW_hh (B rows through prevmap; "none" = row MT, the last one) ---------------------------------------
@pytest.mark.parametrize("B,T", [(42799, 98), (60787, 69)], ids=["MT_4194302_wgrad16", "MT_4194303_tiled"])
def test_wgrad16_limit_hidden_rows_through_prevmap_vs_float64(B, T):
    """hseq is [MT + 1][256]; every row's first token reads its row MT.  (MT + 1) 256 = 2^30 - 256 (wgrad16; row MT ends 1 KB
    below 2^32 bytes) and 2^30 (the tiled product).  Rows have 1 to 3 tokens but the 48 sampled ones, which are full."""
    c = dict(cell="GRU", B=B, T=T, E=64, H=256, layers=1, bi=False)
    MT, H, E = B * T, 256, 64
    name = f"prevmap_MT{MT}"
    assert (MT + 1) * H - 2 ** 30 in (-256, 0)
    rows = np.unique(np.concatenate([[0, B - 1], np.random.RandomState(71).choice(B, eb.MAX_ROWS - 2, replace=False)]))[:eb.MAX_ROWS]
    lens = 1 + np.arange(B, dtype=np.int64) % 3
    lens[rows] = T
    tok_off = eb.tok_offsets(lens)
    print(f"\n[{name}] B = {B}, T = {T}, MT = {MT}, (MT + 1) H = 2^30 {(MT + 1) * H - 2 ** 30:+d}, row MT at byte {MT * H * 4} "
          f"(2^32 {MT * H * 4 - 2 ** 32:+d}); valid tokens {int(tok_off[-1])}; "
          f"{'wgrad16' if (MT + 1) * H < 2 ** 30 else 'the tiled product'} by tt_wgrad16_supported")
    print(f"  sampled rows ({len(rows)}): {rows.tolist()}")
    ws = eb.workspace_bytes("GRU", B, T, E, H, 1, False, 1)
    eb.require_memory(name, workspace=ws, ids=MT * 8, table=30000 * E * 4)
    _train_and_check(name, c, lens, rows, seed=70)


# ---- case 10: a trainable table past 2^32 elements ---------------------------------------------------------------------------------
def test_trainable_table_past_2_32_elements():
    """V E > 2^32: the gradient is zeroed over V E 4 bytes and scattered at id * E; layer 0's dW_ih is on the tiled product.
    The gradient at the used rows against float64; exactly zero everywhere else, row 0 included."""
    V, E = 16_900_000, 256
    name = f"trainable_V{V}_E{E}"
    c = dict(TINY, E=E)
    B, T, H = c["B"], c["T"], c["H"]
    assert V * E > 2 ** 32 and (V - EDGE) * E > 2 ** 32
    print(f"\n[{name}] V E = {V * E} (2^32 {V * E - 2 ** 32:+d}); ids from [1, {EDGE}) and [{V - EDGE}, {V})")
    ws = eb.workspace_bytes("GRU", B, T, E, H, 1, False, 2)
    eb.require_memory(name, table=V * E * 4, gradient=2 * V * E * 4, workspace=ws)
    lens = eb.varied_lens(B, T)
    rows = np.arange(B, dtype=np.int64)
    table = eb.device_table(V, E, 81)
    enc, ids, used, wt, _ = _train_and_check(name, c, lens, rows, V=V, zones=[(1, EDGE), (V - EDGE + 1, V)], table=table,
                                             trainable=True, seed=80)
    assert used[0] == 0 and (used[1:] < EDGE).sum() >= 10 and (used >= V - EDGE).sum() >= 10
    g = enc.embedding.weight.grad
    assert g is not None and tuple(g.shape) == (V, E)
    at_used = g[torch.from_numpy(used).cuda()]
    eb.grad_check(name, "embedding.weight at the used rows", at_used.cpu().numpy(), wt)
    assert not bool(g[0].any()) and not wt[0].any()
    n_all, n_used = eb.nonzero_count(g), int(torch.count_nonzero(at_used))
    print(f"[{name}] non-zero gradient elements: {n_all} in all, {n_used} at the {used.size} used rows")
    assert n_all == n_used > (used.size - 1) * E // 2
    enc.embedding.weight.grad = None
