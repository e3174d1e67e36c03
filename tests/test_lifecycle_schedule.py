"""The continuous-batching plan of tools/run_kitti.py --seqs ... --batch N (schedule()): pure host logic, no device."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _schedule():
    spec = importlib.util.spec_from_file_location("run_kitti", os.path.join(ROOT, "tools", "run_kitti.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.schedule


@pytest.mark.parametrize("lengths, batch", [([5, 3, 7, 1, 4], 2), ([5, 3, 7], 3), ([2, 6], 4), ([4, 0, 3, 3], 1), ([], 2)])
def test_every_frame_once_in_order_and_resets_exactly_on_entry(lengths, batch):
    steps = _schedule()(lengths, batch)
    seen = {i: [] for i in range(len(lengths))}
    slot_seq = [None] * batch
    for active, resets, frames in steps:
        assert len(active) == batch and sorted(frames) == [s for s in range(batch) if active[s]]   # no slot is active without a frame
        assert len(set(resets)) == len(resets)
        for s in range(batch):
            entering = s in frames and frames[s][0] != slot_seq[s]
            assert (s in resets) == entering, (s, resets, frames)     # reset exactly when a new sequence enters the slot
            if s in frames:
                assert not entering or frames[s][1] == 0                # a sequence starts at its first sweep
                slot_seq[s] = frames[s][0]
        for s, (i, k) in frames.items():
            seen[i].append(k)
    for i, n in enumerate(lengths):
        assert seen[i] == list(range(n)), (i, seen[i])                  # every frame once, in order
    if len([n for n in lengths if n]) <= batch:                          # every sequence has a slot of its own: no step is wasted
        assert len(steps) == max(lengths, default=0)


def test_one_slot_runs_the_sequences_back_to_back():
    steps = _schedule()([2, 3], 1)
    assert [f[0] for _, _, f in steps] == [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]
    assert [r for _, r, _ in steps] == [[0], [], [0], [], []]
