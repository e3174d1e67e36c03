"""CPU-side checks of the sequence records (aloam_save_sequences / aloam_load_sequences): the library exports both entries, the ctypes mirror of
aloam_seq_record_header has the layout a C compiler gives the header's, and the time-sliced plan of tools/run_kitti.py --slice (schedule_sliced())."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_kitti():
    spec = importlib.util.spec_from_file_location("run_kitti", os.path.join(ROOT, "tools", "run_kitti.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_library_exports_save_and_load(binding):
    L = binding.lib()
    for name in ("aloam_save_sequences", "aloam_load_sequences"):
        assert name in binding.declared_symbols()
        assert hasattr(L, name)
    out = subprocess.run(["nm", "-D", "--defined-only", binding.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (aloam_[a-z_0-9]+)", out))
    assert {"aloam_save_sequences", "aloam_load_sequences"} <= exported


def test_the_magic_spells_alsq(binding):
    """(The layout of aloam_seq_record_header and the values of the constants are held by test_abi_records.py.)"""
    assert binding.SEQ_RECORD_MAGIC.to_bytes(4, "little") == b"ALSQ"


CASES = [([5, 3, 7, 1, 4], 2, 2), ([5, 3, 7], 3, 1), ([2, 6], 4, 3), ([4, 0, 3, 3], 1, 2), ([], 2, 2), ([6, 6, 6, 6], 2, 2), ([9, 2, 5], 2, 4)]


@pytest.mark.parametrize("lengths, batch, k", CASES)
def test_sliced_plan_runs_every_frame_once_and_swaps_by_save_and_load(lengths, batch, k):
    steps = _run_kitti().schedule_sliced(lengths, batch, k)
    seen = {i: [] for i in range(len(lengths))}
    slot_seq = [None] * batch
    saved = set()                                                      # sequences parked in a record
    ever = set()
    for active, resets, frames, saves, loads in steps:
        assert len(active) == batch and sorted(frames) == [s for s in range(batch) if active[s]]
        assert sum(active) <= batch
        for s, i in saves:                                             # a sequence leaves its slot with frames left: one save
            assert slot_seq[s] == i and len(seen[i]) < lengths[i], (s, i)
            assert i not in saved
            saved.add(i)
            slot_seq[s] = None
        for s, i in loads:                                             # it comes back (into any slot): one load of that record
            assert i in saved and frames[s][0] == i and frames[s][1] == len(seen[i]), (s, i)
            saved.discard(i)
        entered = {s for s in frames if frames[s][0] != slot_seq[s]}
        assert entered == set(resets) | {s for s, _ in loads}, (entered, resets, loads)   # every slot change is a reset (new) or a load (resumed)
        assert not set(resets) & {s for s, _ in loads}
        for s in resets:
            assert frames[s][1] == 0 and frames[s][0] not in ever       # a new sequence starts at its first sweep, once
        for s, (i, f) in frames.items():
            seen[i].append(f)
            slot_seq[s] = i
            ever.add(i)
        resident = [s for s in range(batch) if slot_seq[s] is not None]
        assert len(resident) <= batch
    assert not saved                                                   # nothing is left parked
    for i, n in enumerate(lengths):
        assert seen[i] == list(range(n)), (i, seen[i])                 # every frame once, in order


@pytest.mark.parametrize("lengths, batch", [([5, 3, 7, 1, 4], 2), ([5, 3, 7], 3), ([2, 6], 4), ([4, 0, 3, 3], 1), ([], 2)])
def test_slices_as_long_as_the_longest_sequence_are_schedules_plan(lengths, batch):
    rk = _run_kitti()
    k = max(lengths, default=0) + 1
    for k in (max(1, max(lengths, default=1)), k):
        sliced = rk.schedule_sliced(lengths, batch, k)
        assert [st[:3] for st in sliced] == rk.schedule(lengths, batch)
        assert all(not st[3] and not st[4] for st in sliced)


def test_time_slices_rotate_the_waiting_sequences():
    steps = _run_kitti().schedule_sliced([4, 4, 4], 2, 2)
    assert [sorted(v[0] for v in f.values()) for _, _, f, _, _ in steps][:3] == [[0, 1], [0, 1], [1, 2]]   # sequence 0 waits after 2 frames
    assert steps[2][3] == [(0, 0)] and steps[2][1] == [0]             # saved, and the new sequence 2 takes its slot
    assert any(loads == [(s, 0)] for _, _, _, _, loads in steps for s in range(2))
