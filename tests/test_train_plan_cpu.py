"""The train step's host decisions, without a GPU: which tower runs which recurrence (trainer._towers_in_flight over the pure
trainer._plan_towers), in which order the towers' forward calls go out (trainer._forward_sequence) and what a step specification
refuses (trainer._StepSpec).  These decide co-residency of the column-split recurrences and the order of the ranks' collectives:
a mistake there is a hang, not a wrong number.

The tables below were recorded from the code BEFORE the planner was taken out of _towers_in_flight (commit 38e7007), by driving
that context manager with the stub towers of this file; the forward sequences are read off the loop of that commit's
_train_step_direct, the refusal texts off its _check_negatives.

An outcome is written "QqDd?>QqDd?": the query tower's one_workgroup and one_workgroup_bwd, the document tower's (T, F, N = None),
then "o" when the forward recurrences are to be ordered by events ("-": not); in front of ">" inside the block as entered, behind
it after use_one_workgroup()."""
import types

import pytest
import torch

from twotowermlretrieval_amd import trainer

NEEDS = (0, 32, 64, 128, 192, 256)
ROWS = (8, 16)                       # query tower B rows, document tower 2B
PLAIN = ((False, None), (False, None))   # one_workgroup, one_workgroup_bwd as RNNEncoder sets them

# GRID[(CUs, layers of both towers)][i][j]: query tower needs NEEDS[i] workgroups, document tower NEEDS[j]; towers come in plain
GRID = {
    (64, 1): [
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFTo>FNTN- FNFTo>FNTN- FNFTo>FNTN-",
        "FNFN->FNFN- FNFN->FNFN- FTFNo>TNFN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN-",
        "FNFN->FNFN- FNFTo>FNTN- FTFNo>TNFN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN-",
        "FTFNo>TNFN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN-",
        "FTFNo>TNFN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN-",
        "FTFNo>TNFN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN- FTFTo>TNTN-",
    ],
    (64, 2): [
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNTN->FNTN- FNTN->FNTN- FNTN->FNTN-",
        "FNFN->FNFN- FNFN->FNFN- TNFN->TNFN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN-",
        "FNFN->FNFN- FNTN->FNTN- TNFN->TNFN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN-",
        "TNFN->TNFN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN-",
        "TNFN->TNFN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN-",
        "TNFN->TNFN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN- TNTN->TNTN-",
    ],
    (256, 1): [
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FTFNo>TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FTFNo>TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FTFNo>TNFN- FTFNo>TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFTo>FNTN- FTFNo>TNFN- FTFNo>TNFN-",
        "FNFN->FNFN- FNFTo>FNTN- FNFTo>FNTN- FNFTo>FNTN- FNFTo>FNTN- FTFNo>TNFN-",
    ],
    (256, 2): [
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- TNFN->TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- TNFN->TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- TNFN->TNFN- TNFN->TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNTN->FNTN- TNFN->TNFN- TNFN->TNFN-",
        "FNFN->FNFN- FNTN->FNTN- FNTN->FNTN- FNTN->FNTN- FNTN->FNTN- TNFN->TNFN-",
    ],
    (304, 1): [
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FTFNo>TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FTFNo>TNFN- FTFNo>TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFTo>FNTN- FTFNo>TNFN- FTFNo>TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFTo>FNTN- FNFTo>FNTN- FNFTo>FNTN- FTFNo>TNFN-",
    ],
    (304, 2): [
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- TNFN->TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- TNFN->TNFN- TNFN->TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNFN->FNFN- FNTN->FNTN- TNFN->TNFN- TNFN->TNFN-",
        "FNFN->FNFN- FNFN->FNFN- FNTN->FNTN- FNTN->FNTN- FNTN->FNTN- TNFN->TNFN-",
    ],
}
# (needs, rows or None, CUs, layers, flags the towers come in with, force_one_workgroup) -> outcome
T, F, N = True, False, None
EXTRA = {
    ((192, 192), (8, 16), 256, (1, 1), PLAIN, F): "FTFNo>TNFN-",
    ((192, 192), (8, 16), 256, (2, 2), PLAIN, F): "TNFN->TNFN-",
    ((192, 192), (16, 8), 256, (1, 1), PLAIN, F): "FNFTo>FNTN-",
    ((192, 192), (16, 8), 256, (2, 2), PLAIN, F): "FNTN->FNTN-",
    ((192, 192), (8, 8), 256, (1, 1), PLAIN, F): "FTFNo>TNFN-",
    ((192, 192), (8, 8), 256, (2, 2), PLAIN, F): "TNFN->TNFN-",
    ((256, 256), (8, 16), 256, (1, 1), PLAIN, F): "FTFNo>TNFN-",
    ((256, 256), (8, 16), 256, (2, 2), PLAIN, F): "TNFN->TNFN-",
    ((256, 256), (16, 8), 256, (1, 1), PLAIN, F): "FNFTo>FNTN-",
    ((256, 256), (16, 8), 256, (2, 2), PLAIN, F): "FNTN->FNTN-",
    ((256, 256), (8, 8), 256, (1, 1), PLAIN, F): "FTFNo>TNFN-",
    ((256, 256), (8, 8), 256, (2, 2), PLAIN, F): "TNFN->TNFN-",
    ((192, 192), (8, 16), 304, (1, 1), PLAIN, F): "FTFNo>TNFN-",
    ((192, 192), (8, 16), 304, (2, 2), PLAIN, F): "TNFN->TNFN-",
    ((192, 192), (16, 8), 304, (1, 1), PLAIN, F): "FNFTo>FNTN-",
    ((192, 192), (16, 8), 304, (2, 2), PLAIN, F): "FNTN->FNTN-",
    ((192, 192), (8, 8), 304, (1, 1), PLAIN, F): "FTFNo>TNFN-",
    ((192, 192), (8, 8), 304, (2, 2), PLAIN, F): "TNFN->TNFN-",
    ((256, 256), (8, 16), 304, (1, 1), PLAIN, F): "FTFNo>TNFN-",
    ((256, 256), (8, 16), 304, (2, 2), PLAIN, F): "TNFN->TNFN-",
    ((256, 256), (16, 8), 304, (1, 1), PLAIN, F): "FNFTo>FNTN-",
    ((256, 256), (16, 8), 304, (2, 2), PLAIN, F): "FNTN->FNTN-",
    ((256, 256), (8, 8), 304, (1, 1), PLAIN, F): "FTFNo>TNFN-",
    ((256, 256), (8, 8), 304, (2, 2), PLAIN, F): "TNFN->TNFN-",
    ((128, 256), (8, 16), 256, (2, 1), PLAIN, F): "TNFN->TNFN-",
    ((256, 128), (8, 16), 256, (2, 1), PLAIN, F): "FNTN->FNTN-",
    ((128, 256), (8, 16), 256, (1, 2), PLAIN, F): "TNFN->TNFN-",
    ((256, 128), (8, 16), 256, (1, 2), PLAIN, F): "FNTN->FNTN-",
    ((128, 256), (8, 16), 256, (1, 1), ((T, N), (F, N)), F): "TNFN->TNFN-",
    ((128, 256), (8, 16), 256, (1, 1), ((F, N), (T, N)), F): "FNTN->FNTN-",
    ((128, 256), (8, 16), 256, (1, 1), ((T, T), (F, N)), F): "TTFN->TTFN-",
    ((128, 256), (8, 16), 256, (1, 1), ((F, N), (T, T)), F): "FNTT->FNTT-",
    ((128, 256), (8, 16), 256, (1, 1), ((T, F), (F, N)), F): "TTFNo>TNFN-",
    ((128, 256), (8, 16), 256, (1, 1), ((F, N), (T, F)), F): "FTTFo>TNTF-",
    ((128, 256), (8, 16), 256, (1, 1), ((F, T), (F, N)), F): "FTFNo>TNFN-",
    ((128, 256), (8, 16), 256, (1, 1), ((F, N), (F, T)), F): "FTFTo>TNFT-",
    ((128, 256), (8, 16), 256, (1, 1), ((F, F), (F, N)), F): "FTFNo>TNFN-",
    ((128, 256), (8, 16), 256, (1, 1), ((F, N), (F, F)), F): "FTFFo>TNFF-",
    ((128, 256), (8, 16), 256, (2, 2), ((T, N), (F, N)), F): "TNFN->TNFN-",
    ((128, 256), (8, 16), 256, (2, 2), ((F, N), (T, N)), F): "FNTN->FNTN-",
    ((128, 256), (8, 16), 256, (2, 2), ((T, T), (F, N)), F): "TTFN->TTFN-",
    ((128, 256), (8, 16), 256, (2, 2), ((F, N), (T, T)), F): "FNTT->FNTT-",
    ((128, 256), (8, 16), 256, (2, 2), ((T, F), (F, N)), F): "TNFN->TNFN-",
    ((128, 256), (8, 16), 256, (2, 2), ((F, N), (T, F)), F): "TNTF->TNTF-",
    ((128, 256), (8, 16), 256, (2, 2), ((F, T), (F, N)), F): "TNFN->TNFN-",
    ((128, 256), (8, 16), 256, (2, 2), ((F, N), (F, T)), F): "TNFT->TNFT-",
    ((128, 256), (8, 16), 256, (2, 2), ((F, F), (F, N)), F): "TNFN->TNFN-",
    ((128, 256), (8, 16), 256, (2, 2), ((F, N), (F, F)), F): "TNFF->TNFF-",
    ((192, 192), (8, 16), 256, (1, 1), ((T, N), (F, N)), F): "TNFN->TNFN-",
    ((192, 192), (8, 16), 256, (1, 1), ((F, N), (T, N)), F): "FNTN->FNTN-",
    ((192, 192), (8, 16), 256, (1, 1), ((T, T), (F, N)), F): "TTFN->TTFN-",
    ((192, 192), (8, 16), 256, (1, 1), ((F, N), (T, T)), F): "FNTT->FNTT-",
    ((192, 192), (8, 16), 256, (1, 1), ((T, F), (F, N)), F): "TTFNo>TNFN-",
    ((192, 192), (8, 16), 256, (1, 1), ((F, N), (T, F)), F): "FTTFo>TNTF-",
    ((192, 192), (8, 16), 256, (1, 1), ((F, T), (F, N)), F): "FTFNo>TNFN-",
    ((192, 192), (8, 16), 256, (1, 1), ((F, N), (F, T)), F): "FTFTo>TNFT-",
    ((192, 192), (8, 16), 256, (1, 1), ((F, F), (F, N)), F): "FTFNo>TNFN-",
    ((192, 192), (8, 16), 256, (1, 1), ((F, N), (F, F)), F): "FTFFo>TNFF-",
    ((192, 192), (8, 16), 256, (2, 2), ((T, N), (F, N)), F): "TNFN->TNFN-",
    ((192, 192), (8, 16), 256, (2, 2), ((F, N), (T, N)), F): "FNTN->FNTN-",
    ((192, 192), (8, 16), 256, (2, 2), ((T, T), (F, N)), F): "TTFN->TTFN-",
    ((192, 192), (8, 16), 256, (2, 2), ((F, N), (T, T)), F): "FNTT->FNTT-",
    ((192, 192), (8, 16), 256, (2, 2), ((T, F), (F, N)), F): "TNFN->TNFN-",
    ((192, 192), (8, 16), 256, (2, 2), ((F, N), (T, F)), F): "TNTF->TNTF-",
    ((192, 192), (8, 16), 256, (2, 2), ((F, T), (F, N)), F): "TNFN->TNFN-",
    ((192, 192), (8, 16), 256, (2, 2), ((F, N), (F, T)), F): "TNFT->TNFT-",
    ((192, 192), (8, 16), 256, (2, 2), ((F, F), (F, N)), F): "TNFN->TNFN-",
    ((192, 192), (8, 16), 256, (2, 2), ((F, N), (F, F)), F): "TNFF->TNFF-",
    ((128, 256), N, 256, (1, 1), PLAIN, T): "TNTN->TNTN-",
    ((128, 256), N, 256, (1, 1), ((T, F), (F, T)), T): "TNTN->TNTN-",
    ((128, 256), N, 256, (2, 2), PLAIN, T): "TNTN->TNTN-",
    ((128, 256), N, 256, (2, 2), ((T, F), (F, T)), T): "TNTN->TNTN-",
    ((128, 256), (8, 16), 256, (1, 1), PLAIN, T): "TNTN->TNTN-",
    ((128, 256), (8, 16), 256, (1, 1), ((T, F), (F, T)), T): "TNTN->TNTN-",
    ((128, 256), (8, 16), 256, (2, 2), PLAIN, T): "TNTN->TNTN-",
    ((128, 256), (8, 16), 256, (2, 2), ((T, F), (F, T)), T): "TNTN->TNTN-",
    ((128, 256), N, 256, (1, 1), PLAIN, F): "FNFN->FNFN-",
    ((256, 256), N, 64, (2, 2), ((F, T), (T, F)), F): "FTTF->FTTF-",
}


def _code(v):
    return {True: "T", False: "F", None: "N"}[v]


def _flags(encs):
    return "".join(_code(e.one_workgroup) + _code(e.one_workgroup_bwd) for e in encs)


class _Tower:
    def __init__(self, need, layers, one, one_bwd):
        self.need, self.num_layers, self.dropout = need, layers, 0.0
        self.one_workgroup, self.one_workgroup_bwd, self._status_sink = one, one_bwd, "the caller's sink"
        self.embedding = types.SimpleNamespace(weight=types.SimpleNamespace(is_cuda=True, device="cuda:0"))

    def split_workgroups(self, B):
        return self.need


class _Optimizer(trainer._FlatClipAdam):
    def __init__(self):
        self._pending_status, self._reduced_upto = [], 0

    def watch(self, *encs):
        for e in encs:
            e._status_sink = self._pending_status


def _drive(monkeypatch, needs, rows, cus, layers, flags_in, force):
    """One block of _towers_in_flight over stub towers, left normally and by an exception: {how: (outcome, what is left)}."""
    monkeypatch.setattr(torch.cuda, "get_device_properties", lambda dev: types.SimpleNamespace(multi_processor_count=cus))
    out = {}
    for leave in ("normal", "raise"):
        q, d = (_Tower(n, l, *f) for n, l, f in zip(needs, layers, flags_in))
        model = types.SimpleNamespace(query_encoder=q, doc_encoder=d)
        opt = _Optimizer()
        try:
            with trainer._towers_in_flight(model, opt, {q: rows[0], d: rows[1]} if rows else {}, force) as plan:
                assert q._status_sink is opt._pending_status and d._status_sink is opt._pending_status
                code = _flags((q, d)) + ("o" if plan.needs_order else "-")
                plan.use_one_workgroup()
                code += ">" + _flags((q, d)) + ("o" if plan.needs_order else "-")
                opt._pending_status.append("a status word")
                opt._reduced_upto = 7
                if leave == "raise":
                    raise KeyError("the step died")
        except KeyError:
            pass
        out[leave] = (code, (_flags((q, d)), q._status_sink, d._status_sink, list(opt._pending_status), opt._reduced_upto))
    return out


def _check_block(monkeypatch, case, want):
    needs, rows, cus, layers, flags_in, force = case
    got = _drive(monkeypatch, needs, rows, cus, layers, flags_in, force)
    came_in = "".join(_code(v) for f in flags_in for v in f)
    assert got["normal"][0] == want and got["raise"][0] == want, (case, got)
    # restored on the way out, whichever way; only a step that died leaves no status word and no reduced prefix behind
    assert got["normal"][1] == (came_in, "the caller's sink", "the caller's sink", ["a status word"], 7), (case, got)
    assert got["raise"][1] == (came_in, "the caller's sink", "the caller's sink", [], 0), (case, got)


def _grid_cases():
    for (cus, layers), lines in GRID.items():
        for nq, line in zip(NEEDS, lines):
            for nd, want in zip(NEEDS, line.split()):
                yield ((nq, nd), ROWS, cus, (layers, layers), PLAIN, False), want


@pytest.mark.parametrize("cus,layers", sorted(GRID))
def test_towers_in_flight_decides_as_recorded_on_the_grid(monkeypatch, cus, layers):
    assert [len(line.split()) for line in GRID[(cus, layers)]] == [len(NEEDS)] * len(NEEDS)
    for case, want in _grid_cases():
        if case[2] == cus and case[3][0] == layers:
            _check_block(monkeypatch, case, want)


@pytest.mark.parametrize("case", sorted(EXTRA, key=repr), ids=repr)
def test_towers_in_flight_decides_as_recorded_off_the_grid(monkeypatch, case):
    _check_block(monkeypatch, case, EXTRA[case])


# ---- the planner itself: no towers, no device ------------------------------------------------------------------------------------
def _planned(case):
    """The same outcome from _plan_towers alone, applied to a table of flags the way _towers_in_flight applies it to encoders."""
    needs, rows, cus, layers, flags_in, force = case
    towers = ("query", "doc")
    flags = {t: list(f) for t, f in zip(towers, flags_in)}
    # (what _towers_in_flight gathers: a tower already on the one-workgroup kernels in both directions needs no CU of its own)
    need = {t: 0 if (flags[t][0] and flags[t][1] is not False) else n for t, n in zip(towers, needs)} if rows else {}
    rows = dict(zip(towers, rows)) if rows else {}
    stacked = any(n > 1 for n in layers)

    def apply(plan):
        for t in plan.one_workgroup:
            flags[t] = [True, None]
        for t in plan.one_workgroup_bwd:
            flags[t][1] = True
        return "".join(_code(v) for t in towers for v in flags[t]) + ("o" if plan.ordered else "-")
    if force:
        first = apply(trainer._plan_towers(dict.fromkeys(towers, 0), {}, cus, stacked, "forced"))
        return first + ">" + first
    plan = trainer._plan_towers(need, rows, cus, stacked, "ordered")
    first = apply(plan)
    return first + ">" + (apply(trainer._plan_towers(need, rows, cus, stacked, "no_events")) if plan.ordered else first)


def test_plan_towers_decides_as_recorded():
    cases = list(_grid_cases()) + list(EXTRA.items())
    assert len(cases) == 6 * 36 + len(EXTRA)
    for case, want in cases:
        assert _planned(case) == want, case


def test_plan_towers_changes_nothing_it_was_given():
    need, rows = {"query": 128, "doc": 256}, {"query": 8, "doc": 16}
    for mode in ("ordered", "no_events", "forced"):
        trainer._plan_towers(need, rows, 256, False, mode)
        assert need == {"query": 128, "doc": 256} and rows == {"query": 8, "doc": 16}


# ---- the order of the towers' forward calls --------------------------------------------------------------------------------------
def test_forward_sequence_of_every_order():
    from twotowermlretrieval_amd._lib import TT_ENC_PHASE_BEGIN as BEGIN, TT_ENC_PHASE_FINISH as FINISH
    DOC, QRY = trainer._DOC, trainer._QRY
    assert (DOC, QRY) == (0, 1)      # (the direct step's tuples: document tower, query tower)
    # (tower, phase, what the call does with the ordering event, on the one-workgroup recurrence)
    whole_calls = [(DOC, 0, None, False), (QRY, 0, None, False)]     # the document tower first: the step's critical path
    for order in ("query_first", "query_first_whole", "doc_first", "query_one_wg"):
        assert trainer._forward_sequence(False, order) == whole_calls, order
    # the recording call is issued before the waiting one; the document tower's call in two halves around the query tower's
    assert trainer._forward_sequence(True, "query_first") == [(DOC, BEGIN, None, False), (QRY, 0, "record", False),
                                                              (DOC, FINISH, "wait", False)]
    assert trainer._forward_sequence(True, "query_first_whole") == [(QRY, 0, "record", False), (DOC, 0, "wait", False)]
    assert trainer._forward_sequence(True, "doc_first") == [(DOC, 0, "record", False), (QRY, 0, "wait", False)]
    assert trainer._forward_sequence(True, "query_one_wg") == [(DOC, 0, None, False), (QRY, 0, None, True)]
    assert trainer._FWD_ORDER == "query_first"
    for ordered in (False, True):
        with pytest.raises(ValueError):
            trainer._forward_sequence(ordered, "two_phase")


# ---- what a step specification refuses -------------------------------------------------------------------------------------------
def _spec(negatives, gather_negatives, graphs):
    return trainer._StepSpec(0.2, negatives, 0.05, gather_negatives, True, True).checked(graphs)


def test_step_spec_refusals():
    for negatives in ("paired", "in_batch"):
        for graphs in (False, True):
            spec = _spec(negatives, False, graphs)
            assert spec == (0.2, negatives, 0.05, False, True, True)
    assert _spec("in_batch", True, False).gather_negatives is True
    for bad in ("hard", "", None, "IN_BATCH"):
        for gather in (False, True):
            with pytest.raises(ValueError) as e:
                _spec(bad, gather, False)
            assert str(e.value) == f'negatives must be "paired" or "in_batch", got {bad!r}'
    for graphs in (False, True):
        with pytest.raises(ValueError) as e:
            _spec("paired", True, graphs)
        assert str(e.value) == "gather_negatives=True needs negatives=\"in_batch\", got negatives='paired'"
    with pytest.raises(ValueError) as e:
        _spec("in_batch", True, True)
    assert str(e.value) == ("gather_negatives=True is not available with graphs=True (the exchange of the passages sits between the "
                            "captured forward and backward)")


def test_step_spec_is_frozen():
    spec = _spec("paired", False, False)
    with pytest.raises(AttributeError):
        spec.margin = 0.5
    assert spec._fields == ("margin", "negatives", "temperature", "gather_negatives", "concurrent_towers", "direct")
