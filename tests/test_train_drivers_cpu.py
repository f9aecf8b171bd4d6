"""What the training and evaluation drivers of train.py do, in which order: the epoch loop of the branch, joint and classifier
stages (train, buffers from rank 0, validate, scheduler step, rank 0's report / best / periodic checkpoint, barrier), the
resume path and its refusals, and the preambles of the three evaluators, recorded on the CPU with stand-in models
(tests/_train_transcript.py) single-process and as two gloo ranks, and compared with tests/golden/train_drivers.json."""
import json

import pytest

from tests import _train_transcript as TT


@pytest.fixture(scope="module")
def golden():
    with open(TT.GOLDEN_PATH) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def transcripts():
    """every case runs once; the tests below read what it left"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = TT.run_case(name)
        return cache[name]
    return get


def _events(transcript, kind, rank=0):
    return [e for e in transcript[f"rank{rank}"] if e[0] == kind]


def test_golden_has_exactly_the_cases(golden):
    assert list(golden) == list(TT.CASES)


@pytest.mark.parametrize("name", list(TT.CASES))
def test_transcript_matches_golden(name, golden, transcripts):
    diff = TT.differences(transcripts(name), golden[name], name)
    assert not diff, "\n".join(diff)


@pytest.mark.parametrize("name", [n for n, c in TT.CASES.items() if c[1] == 2])
def test_two_ranks_issue_the_same_collectives_and_only_rank0_writes(name, transcripts):
    t = transcripts(name)
    assert _events(t, "coll", 0) == _events(t, "coll", 1) and len(_events(t, "coll", 0)) > 8
    assert _events(t, "save", 1) == _events(t, "replace", 1) == []
    # (load_pretrained_model speaks on every rank; the epoch report is rank 0's)
    assert [e for e in _events(t, "out", 1) if not e[1].startswith("Checkpoint ")] == [] and _events(t, "out", 0)
    assert [e[1] for e in _events(t, "save", 0)] == [e[2] for e in _events(t, "replace", 0)]
    assert sorted(set(f.rsplit("/", 1)[1] for f in t["files"])) == sorted(set(e[1] for e in _events(t, "save", 0)))
    # the replicas end identical: weights, running statistics, learning rate
    assert _events(t, "return", 0)[-1][-1] == _events(t, "return", 1)[-1][-1]
    assert _events(t, "sched", 0) == _events(t, "sched", 1)


def test_a_rank_without_images_of_the_level_joins_every_step(transcripts):
    t = transcripts("gloo2/branch_rank1_never_holds_the_level")
    assert [e for e in _events(t, "fwd", 1) if e[2]] == []                    # rank 1 never ran a training forward ...
    losses0, state0 = _events(t, "return", 0)[0][1:]
    losses1, state1 = _events(t, "return", 1)[0][1:]
    assert len(losses0) == 10 and losses1 == []                                # ... and took no step of its own,
    assert state0["w"] == state1["w"] == [0.5 + 3 * TT.STEP - 10 * TT.STEP]    # but moved with rank 0 in all ten


def test_nobody_steps_when_no_rank_holds_the_level(transcripts):
    t = transcripts("gloo2/branch_nobody_holds_the_level")
    for rank in (0, 1):
        losses, state = _events(t, "return", rank)[0][1:]
        assert losses == [] and state["w"] == [0.5 + 3 * TT.STEP] and state["bn.num_batches_tracked"] == [0.0]
        assert [e for e in _events(t, "fwd", rank) if e[2]] == []
    assert not any(e[2] == [192] for e in _events(t, "coll"))                  # no gradient bucket went out


def test_single_process_stages_write_best_and_the_fifth_epoch(transcripts):
    for name, sub in (("branch/6_epochs_then_resume", "dehazing/medium/"), ("joint/5_epochs_then_resume", "joint/"),
                      ("classifier/5_epochs_then_evaluate", "classifier/")):
        t = transcripts(name)
        assert t["files"] == [sub + "best_model.pth", sub + "checkpoint_epoch_5.pth"], name
        assert _events(t, "coll") == []


def test_train_and_validation_seeds(transcripts):
    """train seed = seed + epoch, validation always seed + 500000, also after a resume"""
    t = transcripts("branch/6_epochs_then_resume")
    seeds = [e[4] for e in _events(t, "loader")]
    assert seeds == [s for epoch in list(range(6)) + [5, 6] for s in (42 + epoch, 500042)]
