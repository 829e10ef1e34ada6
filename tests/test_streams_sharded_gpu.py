"""Two calls to ONE ShardedIndex in flight on different streams (world 1 on a real RCCL communicator, resident shard,
screen=True).  One issuing thread only: every search of this class is a collective, so there is no two-thread schedule.
Calls of one shape share a slot (send block, receive buffer, outputs) and are ordered by the slot's `merged` event; calls of
different shapes take different slots; submit() has slots of its own.  The held schedule (tests/stream_sched.py) keeps call 1
queued behind a hold on A while call 2 is issued on B: both results must be bit-equal to the same calls made alone.

(The window this class had -- `merged` recorded before the clones that read the slot -- is a few microseconds between two
launches on one stream; no schedule here can hold it open, and it was closed from reading.  These tests pin the ordering
that is there.)  None of these calls synchronises with the host on a resident shard: `early` is asserted for each."""
import socket

import pytest
import torch
import torch.distributed as dist

import stream_sched as ss
import streams_cases as sc

pytestmark = pytest.mark.gpu

K = sc.K


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.fixture(scope="module")
def nccl_group():
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    yield
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def env(nccl_group):
    import twotowermlretrieval_amd as tt
    from twotowermlretrieval_amd import index as _index
    mp = pytest.MonkeyPatch()
    mp.setattr(_index, "SCREEN_MIN_DOCS", 0)
    c = sc.cases()
    sh = c.dress(tt.ShardedIndex.from_global(c.rows.cuda(), shard_k=50, screen=True))
    assert not sh.streamed and sh.collective.startswith("rccl-c-abi"), sh.collective
    # 'a' and 'a2': the same shape (one slot), different rows; 'b': another shape (another slot)
    q = {"a": c.q["a"], "a2": torch.roll(c.q["a"], 7, 0).contiguous(), "b": c.q["b"]}
    match = {"a": c.match["a"], "a2": tuple(torch.roll(t, 7, 0).contiguous() for t in c.match["a"]), "b": c.match["b"]}
    tail = {}
    for s in q:
        v, i = sh.search_after(q[s], K)
        tail[s] = (v[:, -1].clone(), i[:, -1].clone())
    torch.cuda.synchronize()
    calls = {"search": lambda s: sh.search(q[s], K),
             "tagged_search": lambda s: sh.tagged_search(q[s], K, *match[s]),
             "biased_search": lambda s: sh.biased_search(q[s], K),
             "search_after": lambda s: sh.search_after(q[s], K, after=tail[s])}
    wants = {(n, s): ss.serial(lambda: calls[n](s)) for n in calls for s in q}
    yield sh, q, calls, wants
    mp.undo()


def test_serial_sharded_search_is_the_resident_indexes(env):
    import twotowermlretrieval_amd as tt
    sh, q, calls, wants = env
    c = sc.cases()
    ix = c.dress(tt.BruteForceIndex(c.rows.cuda()))
    for n in ("search", "tagged_search", "biased_search"):
        assert ss.same(wants[(n, "b")], ss.serial(lambda: sc.CALLS[n](ix, c, "b"))), n


@pytest.mark.parametrize("name", ["search", "tagged_search", "biased_search", "search_after"])
def test_held_schedule_same_shape_one_slot(env, name):
    sh, q, calls, wants = env
    h = ss.held(lambda: calls[name]("a"), lambda: calls[name]("a2"))
    print(f"sharded {name} a -> a2: early={h.early} late={h.late} overlapped={h.overlapped}")
    assert h.early, f"ShardedIndex.{name} became synchronous"
    assert ss.same(h.r1, wants[(name, "a")]), f"{name} (held on A) differs from the serial result"
    assert ss.same(h.r2, wants[(name, "a2")]), f"{name} (on B, same slot) differs from the serial result"


@pytest.mark.parametrize("first,second", [("search", "search"), ("tagged_search", "search_after"), ("biased_search", "search")])
def test_held_schedule_different_shapes_different_slots(env, first, second):
    sh, q, calls, wants = env
    h = ss.held(lambda: calls[first]("a"), lambda: calls[second]("b"))
    assert h.early, f"ShardedIndex.{first} became synchronous"
    assert ss.same(h.r1, wants[(first, "a")]) and ss.same(h.r2, wants[(second, "b")])


def test_submit_held_then_search_then_result(env):
    """submit() on A behind the hold; search() on B issues the step's deferred exchange first (one issue order on every rank),
    on the exchange stream, where it waits for A; .result() then hands out the submitted step's rows."""
    sh, q, calls, wants = env
    h = ss.held(lambda: sh.submit(q["a"], K), lambda: sh.search(q["a2"], K))
    assert h.early, "ShardedIndex.submit became synchronous"
    pv, pi = h.r1.result()
    ss.drain(torch.cuda.current_stream())
    assert ss.same((pv, pi), wants[("search", "a")]), "submit().result() differs from the serial search"
    assert ss.same(h.r2, wants[("search", "a2")]), "search (on B, behind a held submit) differs from the serial result"
