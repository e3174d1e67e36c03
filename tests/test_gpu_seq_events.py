"""Per-sequence host state with every opt-in feature on at once (capi_seq.hip; DESIGN.md §7b, the table of events): one context with mapping,
the map spill, place recognition and the default grid overlap, batch 3.  After three frames one event is applied to slot 1 only, and each
event re-injects the state the slot already had - its own last clouds, its own cubes, its own frame, its own record - so the remaining frames
of all three slots must equal, bit for bit and in every getter, those of a twin that was left alone: any difference is a flag the event left
stale or cleared by mistake.  Slot 1 is frozen from the third frame on in both runs: its map then takes no insertion, so a re-injected map
(which packs the pool anew) cannot change the compaction count, and the refusal of aloam_score_map_corrections after an event is the event's
doing (the same call is accepted right before it).  The count of pool compactions is compared too, except where the event changes what it
depends on: the size of the pools (all slots, after the growth) and the packing of a slot's pool row (the loaded slot, as in test_gpu_checkpoint.full)."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_checkpoint import full, last_sizes, make
from test_gpu_localization import cubes, frame
from test_gpu_sequence_lifecycle import diff

pytestmark = pytest.mark.gpu
B, F, FIRST, POOL = 3, 8, 3, 16384
FROZEN = [False, True, False]
EVENTS = ["set_last", "set_map", "set_map_frame", "pool_growth", "reset_and_load"]


def _drives(sequence):
    got = [sequence("VLP-16", F, seed=41 + 7 * i, columns=256) for i in range(B)]
    return [g[0] for g in got], got[0][3]


def _context(binding, sequence):
    drives, model = _drives(sequence)
    g = make(binding, model, B, max(len(x) for d in drives for x in d) + 64, True, pool=POOL)
    g.map_spill_enable(64, POOL)
    g.places_enable(B * F)
    return g, drives


def _frames(binding, g, drives, first, last, loaded=False):
    """Frames first .. last - 1, a place added per slot and frame; {(frame, slot): snapshot}.  loaded: slot 1 holds a record, compared as the
    record tests compare one (test_gpu_checkpoint.full: the residue past the previous last clouds and the compaction count are not its)."""
    out = {}
    for k in range(first, last):
        prev = last_sizes(binding, g, 1)
        frame(g, [d[k] for d in drives], frozen=FROZEN if k >= FIRST - 1 else None)
        g.places_add(range(B))
        g.synchronize()
        for b in range(B):
            out[(k, b)] = full(binding, g, b, True, prev if loaded and b == 1 else None)
            out[(k, b)]["compactions"] = g.map_info(b)["compactions"]
        out[(k, "record")] = full(binding, g, 1, True, prev)
    out["places"] = g.places_export().tobytes()
    out["spill"] = [repr(g.map_spill_info(b)) for b in range(B)]
    return out


@pytest.fixture(scope="module")
def twin(binding, sequence):
    g, drives = _context(binding, sequence)
    _frames(binding, g, drives, 0, FIRST)
    out = _frames(binding, g, drives, FIRST, F)
    g.close()
    return out


@pytest.mark.parametrize("event", EVENTS)
def test_an_event_that_reinjects_a_slots_own_state_changes_nothing(binding, sequence, twin, event):
    g, drives = _context(binding, sequence)
    _frames(binding, g, drives, 0, FIRST)
    p = g.map_pose(1)
    cand = binding.map_corrections(p["q_wmap_wodom"][None], p["t_wmap_wodom"][None])
    import torch
    sc, best = torch.zeros(32, dtype=torch.uint8).pin_memory(), torch.zeros(1, dtype=torch.int32).pin_memory()

    def score():
        return binding.lib().aloam_score_map_corrections(g.h, (C.c_int * 1)(1), 1, C.c_void_p(cand.ctypes.data), 1, C.c_void_p(sc.data_ptr()), C.c_void_p(best.data_ptr()))

    assert score() == 0                                                    # slot 1 has just taken a frozen step
    g.synchronize()
    if event == "set_last":
        g.set_last(g.cloud(binding.CLOUD_CORNER_LAST, 1), g.cloud(binding.CLOUD_SURF_LAST, 1), seq=1)
    elif event == "set_map":
        for cls, own in enumerate(cubes(g, 1)):
            g.set_map(own, cls, seq=1)
        assert score() == binding.E_STATE
    elif event == "set_map_frame":
        i = g.map_info(1)
        g.set_map_frame((i["cenW"], i["cenH"], i["cenD"]), p["q_wmap_wodom"], p["t_wmap_wodom"], i["frame_count"], seq=1)
        assert score() == binding.E_STATE
    elif event == "pool_growth":
        own, before = cubes(g, 1)[0], g.map_pool_info()
        g.set_map({0: np.zeros((before["pool_points"] + 1, 4), np.float32)}, 0, seq=1)
        assert g.map_pool_info()["growths"] > before["growths"]
        g.set_map(own, 0, seq=1)                                           # its own corner cubes again, in the pool that grew
        assert score() == binding.E_STATE
    else:
        blob, off = g.save_sequences([1])
        g.reset_sequences([1])
        g.load_sequences([1], blob, off)
        assert score() == binding.E_STATE
        g.set_active(None)
        assert binding.lib().aloam_mapping_step(g.h) == binding.E_STATE   # loaded, and no odometry step yet: it may not map
        assert "sequence 1" in binding.lib().aloam_last_error(g.h).decode()
    got = _frames(binding, g, drives, FIRST, F, loaded=event == "reset_and_load")
    g.close()
    for k in range(FIRST, F):
        for b in range(B):
            loaded = event == "reset_and_load" and b == 1
            want = twin[(k, "record")] if loaded else twin[(k, b)]
            differ = [x for x in diff(got[(k, b)], want) if x != "compactions" or not (loaded or event == "pool_growth")]
            assert not differ, (event, "frame", k, "slot", b, differ)
    assert got["places"] == twin["places"], event
    assert got["spill"] == twin["spill"], event
