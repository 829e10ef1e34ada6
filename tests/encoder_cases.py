"""The encoder / training dispatch table as test cases, one per dispatch class (tests only; shared by
test_encoder_f64_cpu.py and test_encoder_f64_gpu.py).

Entry: (id, cell, B, T, E, H, layers, bi, flags).  The shape decides which kernel runs a product:
  input projection   gemm_rows16 narrow (ceil(K/16) in {13, 16, 19}, N % 64 == 0) / wide (ceil(K/16) == 32, N % 32 == 0), both
                     N >= 256 (gemm_rows16.hip: tt_gemm_rows16_supported); otherwise the tiled f16-split GEMM (sgemm.hip)
  recurrence         GRU H = 128 / 256: gru16x4 (B <= 1024) or gru16; otherwise the fp32 gru_seq_kernel<8 | 16, cell>
  weight gradients   wgrad16 (rows 3H | 4H | H a multiple of 256, N >= 64; the 5-tile form for 256 < N <= 320) or the tiled GEMM
  projection head    two GEMMs from B >= 2048; its gradient split-K from B >= 256
  prep               fused when B <= 1024 and B T <= 8192
Every comment names the predicate the case sits on and the kernel it is meant to reach.  "gru16x4" assumes a 256-CU device
(the column-split recurrence needs its teams co-resident); on a smaller device the same case runs gru16.

flags: V (default 300), zero_inside (default 0.05), arith ("f32"), trainable (the table is a parameter), gen_T / full_row
(ids generated at gen_T columns, zero columns appended up to T)."""
from __future__ import annotations

import zlib

import numpy as np

import synth

V_DEFAULT = 300

CASES = [
    # ---- narrow gemm_rows16 ----------------------------------------------------------------------------------------
    ("a1", "GRU", 9, 11, 196, 128, 1, False, {}),    # 13 k-steps, partial last; N=384: 6 chunks on 4 waves; gemm_rows16_kernel<13,false>
    ("a2", "GRU", 3, 5, 208, 256, 1, False, {}),     # 13 k-steps, full; serving-size batch: the tail split engages; gru16x4
    ("a3", "GRU", 9, 11, 244, 512, 1, False, {}),    # 16 k-steps, partial; N=1536: 6 passes per wave; gru_seq_kernel<16,GRU> + gru_bwd_seq_kernel<16,GRU>; wgrad16 M=1536
    ("a4", "LSTM", 9, 11, 292, 64, 1, False, {}),    # 19 k-steps, partial; N=256 the minimum, one chunk per wave; wgrad16_kernel<5,true> M=256 N=292
    ("a5", "LSTM", 9, 11, 304, 192, 1, False, {}),   # 19 k-steps, full; N=768; 6-wave recurrence gru_seq_kernel<8,LSTM>
    ("a6", "RNN", 9, 11, 256, 320, 1, False, {}),    # 16 k-steps; N=320: 5 chunks on 4 waves; gru_seq_kernel<16,RNN> with 10 waves
    # ---- wide gemm_rows16 ------------------------------------------------------------------------------------------
    ("b1", "GRU", 9, 11, 500, 96, 1, False, {}),     # 32 k-steps, partial; N=288: 9 chunks on 8 waves; gemm_rows16_kernel<32,true>
    ("b2", "GRU", 9, 11, 512, 256, 1, False, {}),    # wide form as layer 0, per-row scaling; gru16x4; wgrad16 N=512
    ("b3", "LSTM", 5, 7, 512, 256, 2, True, {}),     # layer 1 wide at N=1024; no tail split
    ("b4", "RNN", 9, 11, 300, 256, 2, True, {}),     # layer 1 wide at N=256: one chunk per wave
    ("b5", "GRU", 5, 7, 512, 160, 1, False, {}),     # N=480: 15 chunks on 8 waves
    # ---- just outside the rows16 predicates: tiled sgemm16 with pre-split B -----------------------------------------
    ("c1", "GRU", 7, 9, 192, 256, 1, False, {}),     # 12 k-steps: below the narrow set; K = 192 a k-tile multiple
    ("c2", "GRU", 7, 9, 260, 256, 1, False, {}),     # 17 k-steps; K padded to 288; wgrad16 N=260 just over a tile edge
    ("c3", "GRU", 7, 9, 308, 256, 1, False, {}),     # 20 k-steps: one past the north-star's 19
    ("c4", "GRU", 7, 9, 496, 256, 1, False, {}),     # 31 k-steps: one below the wide form
    ("c5", "GRU", 7, 9, 516, 256, 1, False, {}),     # 33 k-steps: one past the wide form
    ("c6", "GRU", 9, 11, 300, 160, 1, False, {}),    # N=480 is no multiple of 64; 5-wave recurrence; tiled weight gradients
    ("c7", "GRU", 9, 11, 4, 32, 1, False, {}),       # both minima: K=4 in a 32-wide k-tile, N=96
    ("c8", "GRU", 9, 11, 36, 224, 1, False, {}),     # 7-wave recurrence
    ("c9", "LSTM", 5, 7, 1024, 480, 1, True, {}),    # K > 512; gru_seq_kernel<16,LSTM> with 15 waves; N=1920
    ("c10", "LSTM", 5, 7, 60, 512, 1, False, {}),    # <16,LSTM> forward and backward at the largest LDS; dW_ih tiled (N=60 < 64) beside wgrad16 dW_hh
    ("c11", "GRU", 5, 7, 68, 448, 1, False, {}),     # 14-wave gru_seq_kernel<16,GRU>; 3H = 1344 is no multiple of 256: tiled weight gradients
    ("c12", "GRU", 9, 11, 32, 256, 1, False, {}),    # dW_ih tiled (N=32), dW_hh wgrad16
    # ---- wgrad16 tile edges (N = E at layer 0; 260 is c2); four instantiations: 4 / 5 column tiles per wave x B rows direct / mapped ----
    ("w1", "GRU", 7, 9, 64, 256, 1, False, {}),      # N=64: the smallest wgrad16 takes
    ("w2", "GRU", 7, 9, 68, 256, 1, False, {}),      # N=68: a 4-column tail
    ("w3", "GRU", 7, 9, 132, 256, 1, False, {}),     # N=132: just over one 128 tile
    ("w4", "GRU", 7, 9, 320, 256, 1, False, {}),     # N=320: the widest 5-tile form, two full 160 tiles
    ("w5", "GRU", 7, 9, 324, 256, 1, False, {}),     # N=324: back on 128 tiles, 4-column tail
    # the 5-tile form with B rows direct is an upper layer's dW_ih at 256 < ndir H <= 320 with gates H a multiple of 256: LSTM H=320 only
    ("w6", "LSTM", 5, 7, 64, 320, 2, False, {}),     # wgrad16_kernel<5,false> (layer 1: M=1280, N=320); gru_seq_kernel<16,LSTM> with 10 waves
]
# ---- token-count edges: B=1, row 0 full, so the count is exact ------------------------------------------------------
for _T in (1, 63, 64, 65, 127, 128, 129):
    CASES.append((f"tA{_T}", "GRU", 1, _T, 300, 256, 1, False, {"zero_inside": 0.0}))  # token-stationary K1, gru16x4, wgrad16 (one token < K slabs at T=1)
for _T in (1, 63, 64, 65, 127, 128, 129):
    CASES.append((f"tB{_T}", "GRU", 1, _T, 52, 64, 1, False, {"zero_inside": 0.0}))    # all-tiled path
CASES += [
    # ---- row-group and launch edges ---------------------------------------------------------------------------------
    ("r1_16", "GRU", 16, 5, 300, 256, 1, False, {}),     # one full row group
    ("r1_17", "GRU", 17, 5, 300, 256, 1, False, {}),     # a second group of one row
    ("r2", "GRU", 129, 4, 300, 256, 1, False, {}),       # 9 row groups round up to 2 x 32 CUs
    ("r3", "GRU", 1024, 4, 300, 256, 1, True, {}),       # one split launch per direction
    ("r4", "GRU", 1040, 3, 300, 256, 1, False, {}),      # above the split range: one-workgroup gru16, three-kernel prep
    ("r5", "GRU", 130, 64, 52, 64, 1, False, {}),        # 8320 ids with B <= 1024: three-kernel prep
    ("r6", "GRU", 9, 16, 300, 256, 1, False, {"gen_T": 11, "full_row": False}),   # no row reaches T
    ("r7", "GRU", 2048, 3, 52, 128, 1, True, {}),        # head as two GEMMs behind the f16 recurrence
    ("r8_255", "GRU", 255, 3, 20, 64, 1, True, {}),      # projection gradient: last one-pass size
    ("r8_256", "GRU", 256, 3, 20, 64, 1, True, {}),      # projection gradient: first split-K size
    # ---- arith="f32": a3, b2, c6 again on the fp32-MFMA kernels -------------------------------------------------------
    ("f1", "GRU", 9, 11, 244, 512, 1, False, {"arith": "f32"}),
    ("f2", "GRU", 9, 11, 512, 256, 1, False, {"arith": "f32"}),
    ("f3", "GRU", 9, 11, 300, 160, 1, False, {"arith": "f32"}),
    # ---- trainable table ------------------------------------------------------------------------------------------------
    ("g1", "GRU", 9, 11, 300, 256, 1, False, {"V": 40, "zero_inside": 0.1, "trainable": True}),   # ids collide in the scatter; sgemm16<false,true> input gradient N=300
    ("g2", "LSTM", 9, 11, 36, 64, 2, True, {"V": 40, "zero_inside": 0.1, "trainable": True}),     # table gradient behind the LSTM
]

IDS = [c[0] for c in CASES]
BY_ID = {c[0]: c for c in CASES}
GATES = {"GRU": 3, "LSTM": 4, "RNN": 1}


def make_inputs(case):
    """(ids [B,T] int64, table [V,E] f32, state dict, d_out [B,H] f32) of a case, from seeds fixed by its id."""
    cid, cell, B, T, E, H, layers, bi, flags = case
    seed = 1000 + zlib.crc32(cid.encode()) % 100000
    V = flags.get("V", V_DEFAULT)
    gen_T = flags.get("gen_T", T)
    ids = synth.make_ids(seed + 2, B, gen_T, V, zero_inside=flags.get("zero_inside", 0.05), full_row=flags.get("full_row", True))
    if gen_T < T:
        ids = np.concatenate([ids, np.zeros((B, T - gen_T), dtype=np.int64)], axis=1)
    table = synth.make_table(seed, V, E)
    sd = synth.make_encoder_state(seed + 1, E, H, layers, bi, gates=GATES[cell])
    d_out = np.random.RandomState(seed + 3).standard_normal((B, H)).astype(np.float32)
    return np.ascontiguousarray(ids), table, sd, d_out
