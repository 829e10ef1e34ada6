"""The sequence of library calls behind every public method of the index classes is pinned (tests/call_trace.py).

tests/golden/index_call_trace.json was written by `python tests/call_trace.py --write` on the tree of the commit its header
names, before the index classes' host code was folded into shared pieces (one mode table, one streamed walk, one exchange
step); this tree must make the same calls: the same names in the same order, every scalar argument, which pointers are
null, and the same refusals with the same words.  Workspace sizes are recorded as "size" (they depend on the CU count).

Shapes, the smallest at which every branch is taken: 200 x 64 rows numbered from 7, B = 3, k = 5 (and k = 100: the large
route), fp32 and bf16; a StreamedIndex over them with block_docs = 64 (four word-aligned blocks, the last of 8 rows) and with
block_docs = 50 (biased search pads its slices; masked, tagged and masked-count calls are refused); world-1 ShardedIndex
over the resident and the streamed rows with shard_k = 16; 4096 x 256 rows screened (SCREEN_MIN_DOCS = 0 as in the
cross-stream tests), plain and screen_masked=True, a world-1 ShardedIndex over them (seed list + seeded calls), and a
StreamedIndex over 5096 x 256 rows with block_docs = 4096, whose two blocks (4096 and 1000 rows) take the screened route.
"""
import json

import pytest

import call_trace

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def traces():
    return call_trace.index_traces()


def test_the_trace_file_names_its_commit():
    assert len(json.loads(call_trace.TRACE_FILE.read_text())["commit"]) >= 7


def test_every_public_call_makes_the_recorded_library_calls(traces):
    want = json.loads(call_trace.TRACE_FILE.read_text())["traces"]
    got = json.loads(json.dumps(traces))  # (tuples and floats as the file holds them)
    assert list(got) == list(want)
    different = []
    for label in want:
        if got[label] != want[label]:
            n = next((j for j, (a, b) in enumerate(zip(got[label], want[label])) if a != b), min(len(got[label]), len(want[label])))
            different.append(f"{label}: call {n}: got {got[label][n:n + 1]}, recorded {want[label][n:n + 1]} "
                             f"({len(got[label])} calls against {len(want[label])})")
    assert not different, "\n".join(different)
