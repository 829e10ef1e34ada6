"""train_step / GraphedTrainStep / DataParallelTrainer with symmetric=: the symmetric "in_batch" loss through the direct step,
the autograd step, a captured graph (with and without labels) and two data-parallel ranks (gloo, two processes on the one GPU,
as tests/test_in_batch_train_gpu.py); symmetric=0.0 stays the plain "in_batch" step."""
import copy
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import synth
from conftest import GOLDEN, ROOT
from test_in_batch_train_gpu import B, TEMP, _free_port, batch, small_model

pytestmark = pytest.mark.gpu


def test_the_step_is_the_step_built_from_the_autograd_form():
    """The direct step, the autograd step (in_batch_softmax_loss(..., symmetric=0.5) inside train_step) and the same step put
    together by hand -- encode, loss, backward, optimizer.step() -- on copies of one model.  The first two are the same launches
    (the same bits, as for the plain loss); the hand-made one to the tolerance of the one-process reproduction in
    tests/test_in_batch_train_gpu.py (2e-6 on the parameters, 1e-6 on the loss)."""
    import twotowermlretrieval_amd as tt
    m1 = small_model()
    m2, m3 = copy.deepcopy(m1), copy.deepcopy(m1)
    o1, o2, o3 = (tt.FusedClipAdam(m.parameters(), lr=1e-2, max_norm=1.0) for m in (m1, m2, m3))
    start = o1.flat_params.clone()
    for step in range(2):
        ids = batch(460 + 3 * step)
        l1 = tt.train_step(m1, o1, *ids, direct=True, negatives="in_batch", temperature=TEMP, symmetric=0.5)
        l2 = tt.train_step(m2, o2, *ids, direct=False, negatives="in_batch", temperature=TEMP, symmetric=0.5)
        o3.zero_grad()
        emb = (m3.encode_query(ids[0]), m3.encode_document(ids[1]), m3.encode_document(ids[2]))
        l3 = tt.in_batch_softmax_loss(emb, temperature=TEMP, symmetric=0.5)
        l3.backward()
        o3.step()
        torch.cuda.synchronize()
        assert float(l1) == float(l2) and np.isfinite(float(l1))
        assert abs(float(l1) - float(l3.detach())) < 1e-6
        if step == 0:        # (the models' own embeddings: the step's loss is the symmetric loss, not the plain one)
            with torch.no_grad():
                plain = tt.in_batch_softmax_loss(tuple(e.detach() for e in emb), temperature=TEMP)
                dirs = tt.symmetric_contrastive_losses(emb[0].detach(), torch.cat(emb[1:]).detach(), 0, TEMP)
            assert float(dirs[0]) == float(plain) and abs(float(l3.detach()) - 0.5 * (float(dirs[0]) + float(dirs[1]))) < 1e-6
            assert abs(float(l1) - float(plain)) > 1e-3
    assert not torch.equal(o1.flat_params, start)
    assert torch.equal(o1.flat_params, o2.flat_params)
    assert torch.equal(o1.exp_avg, o2.exp_avg) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)
    np.testing.assert_allclose(o3.flat_params.detach().cpu().numpy(), o1.flat_params.detach().cpu().numpy(), rtol=0, atol=2e-6)


@pytest.mark.parametrize("direct", [True, False], ids=["direct", "autograd"])
def test_symmetric_0_is_the_plain_in_batch_step(direct):
    import twotowermlretrieval_amd as tt
    m1 = small_model()
    m2 = copy.deepcopy(m1)
    o1 = tt.FusedClipAdam(m1.parameters(), lr=1e-2, max_norm=1.0)
    o2 = tt.FusedClipAdam(m2.parameters(), lr=1e-2, max_norm=1.0)
    ids = batch(470)
    l1 = tt.train_step(m1, o1, *ids, direct=direct, negatives="in_batch", temperature=TEMP, symmetric=0.0)
    l2 = tt.train_step(m2, o2, *ids, direct=direct, negatives="in_batch", temperature=TEMP)
    torch.cuda.synchronize()
    assert float(l1) == float(l2) and torch.equal(o1.flat_params, o2.flat_params) and torch.equal(o1.exp_avg_sq, o2.exp_avg_sq)


@pytest.mark.parametrize("grouped", [False, True], ids=["plain", "grouped"])
def test_graphed_step_equals_the_eager_step_on_padded_ids(grouped):
    """The shapes of the graph test in tests/test_in_batch_train_gpu.py; symmetric is an argument of the captured loss."""
    import twotowermlretrieval_amd as tt
    Vg, Eg, Hg, Bg = 300, 300, 256, 64
    torch.manual_seed(9)
    m = tt.TwoTowerModel({"VOCAB_SIZE": Vg, "EMBED_DIM": Eg, "HIDDEN_DIM": Hg}, synth.make_table(4, Vg, Eg)).cuda().train()
    ref = copy.deepcopy(m)
    opt = tt.FusedClipAdam(m.parameters(), lr=1e-3, max_norm=1.0)
    ref_opt = tt.FusedClipAdam(ref.parameters(), lr=1e-3, max_norm=1.0)
    before = opt.flat_params.clone()
    step = tt.GraphedTrainStep(m, opt, batch=Bg, q_width=16, doc_width=48, negatives="in_batch", temperature=TEMP, grouped=grouped,
                               symmetric=0.5)
    torch.cuda.synchronize()
    assert torch.equal(opt.flat_params, before) and opt.step_count == 0     # warm-up and capture ran on all-padding ids: gate closed

    def padded(t, w):
        out = torch.zeros((t.shape[0], w), dtype=torch.int64, device=t.device)
        out[:, : t.shape[1]] = t
        return out
    groups = (torch.arange(Bg, device="cuda") // 4).to(torch.int64)
    for i, widths in enumerate(((7, 20, 25), (16, 48, 31))):
        ids = [torch.from_numpy(synth.make_ids(500 + 3 * i + s, Bg, T, Vg)).cuda() for s, T in enumerate(widths)]
        kw = dict(groups=groups, neg_groups=None if i == 0 else groups.flip(0).contiguous()) if grouped else {}
        loss = step(*ids, **kw)
        ref_loss = tt.train_step(ref, ref_opt, padded(ids[0], 16), padded(ids[1], 48), padded(ids[2], 48), negatives="in_batch",
                                 temperature=TEMP, symmetric=0.5, **kw)
        torch.cuda.synchronize()
        assert float(loss) == float(ref_loss) and np.isfinite(float(loss))
        assert torch.equal(opt.flat_params, ref_opt.flat_params) and torch.equal(opt.exp_avg_sq, ref_opt.exp_avg_sq)
        assert opt.step_count == ref_opt.step_count == i + 1
    assert not torch.equal(opt.flat_params, before)


def test_what_does_not_combine_is_refused_before_any_launch():
    import twotowermlretrieval_amd as tt
    m = small_model()
    opt = tt.FusedClipAdam(m.parameters(), lr=1e-2)
    before = opt.flat_params.clone()
    ids = batch(480)
    targets = torch.eye(B, 2 * B, device="cuda")
    with pytest.raises(ValueError, match="targets and symmetric"):
        tt.train_step(m, opt, *ids, negatives="in_batch", targets=targets, symmetric=0.5)
    with pytest.raises(ValueError, match="targets and symmetric"):
        tt.DataParallelTrainer(m, negatives="in_batch", symmetric=0.5).step(*ids, targets=targets)
    with pytest.raises(ValueError, match="soft=True and symmetric"):
        tt.GraphedTrainStep(m, opt, batch=B, q_width=16, doc_width=48, negatives="in_batch", soft=True, symmetric=0.5)
    with pytest.raises(ValueError, match="gather_negatives=True"):
        tt.train_step(m, opt, *ids, negatives="in_batch", gather_negatives=True, symmetric=0.5)
    with pytest.raises(ValueError, match='needs negatives="in_batch"'):
        tt.train_step(m, opt, *ids, symmetric=0.5)
    torch.cuda.synchronize()
    assert torch.equal(opt.flat_params, before) and opt.step_count == 0


# ---- two data-parallel ranks -------------------------------------------------------------------------------------------------
def _dp_worker(rank, world, port, tmp):
    sys.path[:0] = [str(ROOT), str(GOLDEN)]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=__import__("datetime").timedelta(seconds=120))
    torch.cuda.set_device(0)
    import twotowermlretrieval_amd as tt
    dev = torch.device("cuda", 0)
    torch.manual_seed(rank)               # the ranks start from DIFFERENT weights; rank 0's are broadcast
    m = tt.TwoTowerModel({"VOCAB_SIZE": 60, "EMBED_DIM": 20, "HIDDEN_DIM": 32}, synth.make_table(3, 60, 20)).to(dev)
    tr = tt.trainer.DataParallelTrainer(m, lr=1e-3, margin=0.5, negatives="in_batch", temperature=TEMP, symmetric=0.5)
    tr.broadcast_parameters()
    ids = [torch.from_numpy(synth.make_ids(40 + s, 8, T, 60)) for s, T in enumerate((5, 9, 7))]
    loss = tr.step(*(x[rank * 4:rank * 4 + 4].to(dev) for x in ids))
    torch.cuda.synchronize()
    np.savez(os.path.join(tmp, f"sym{rank}.npz"), params=tr.optimizer.flat_params.detach().cpu().numpy(), loss=float(loss.item()))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_average_their_local_symmetric_gradients(tmp_path):
    """Rank-local negatives: each rank's two softmaxes run over its own 4 queries and 2 x 4 passages; the all-reduced gradient is
    the mean of the two.  One process reproduces it as the gradient of the mean of the two shard losses (the tolerances of the
    in-batch two-rank test)."""
    import twotowermlretrieval_amd as tt
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "sym0.npz"), np.load(tmp_path / "sym1.npz")
    assert np.array_equal(r0["params"], r1["params"])
    torch.manual_seed(0)
    m = tt.TwoTowerModel({"VOCAB_SIZE": 60, "EMBED_DIM": 20, "HIDDEN_DIM": 32}, synth.make_table(3, 60, 20)).cuda().train()
    opt = tt.FusedClipAdam(m.parameters(), lr=1e-3, max_norm=1.0)
    ids = [torch.from_numpy(synth.make_ids(40 + s, 8, T, 60)).cuda() for s, T in enumerate((5, 9, 7))]
    opt.zero_grad()
    q, p, n = m.encode_query(ids[0]), m.encode_document(ids[1]), m.encode_document(ids[2])
    shard = [tt.in_batch_softmax_loss((q[lo:lo + 4], p[lo:lo + 4], n[lo:lo + 4]), temperature=TEMP, symmetric=0.5) for lo in (0, 4)]
    plain = [tt.in_batch_softmax_loss((q[lo:lo + 4], p[lo:lo + 4], n[lo:lo + 4]), temperature=TEMP) for lo in (0, 4)]
    (0.5 * (shard[0] + shard[1])).backward()
    opt.step()
    torch.cuda.synchronize()
    shard, plain = [float(x.detach()) for x in shard], [float(x.detach()) for x in plain]
    assert abs(shard[0] - float(r0["loss"])) < 1e-6 and abs(shard[1] - float(r1["loss"])) < 1e-6
    assert abs(shard[0] - plain[0]) > 1e-3          # (the ranks did take the symmetric loss)
    np.testing.assert_allclose(opt.flat_params.detach().cpu().numpy(), r0["params"], rtol=0, atol=2e-6)
