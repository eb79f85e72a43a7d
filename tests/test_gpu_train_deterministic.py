"""RN_TRAIN_DETERMINISTIC=1: two runs of a training step sequence from the same seeds give the same BITS -- every parameter, every
Adam moment and the last step's table gradients -- on each fused route, eager and replayed from a graph.  Without the switch the
table gradients (and the audio nets') are sums of float atomics and differ from run to run in their last bits.

The scene is tests/test_gpu_step_routes.py::run_route's: 64x64, 1024 rays, no occupancy refresh, three steps of the first window,
then mean_count = 12000 and two budgeted steps (with a GraphedTrainer: the capture with its first replay, then a second replay)."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HEAD, CAMERA, TORSO = dict(torso=False), dict(torso=False, train_camera=True), dict(torso=True)
# name -> (default_opt overrides, environment beside the switch, GraphedTrainer?)
ROUTES = {
    "head": (HEAD, {}, False),
    "camera_fused": (CAMERA, {"RN_TRAIN_CAMERA": "fused"}, False),
    "torso_fused": (TORSO, {"RN_TORSO_TRAIN": "fused"}, False),
    "graph_head": (HEAD, {}, True),
}
_RUNS = {}


def _set_environment(env, monkeypatch):
    for name in [n for n in os.environ if n.startswith("RN_")]:
        monkeypatch.delenv(name)
    monkeypatch.setenv("RN_TRAIN_NOISE", "torch")            # the seeded jitter, as conftest pins it for every test
    monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", "1")
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _run(name, mean_counts=(12000,)):
    """-> {array name: uint32 bits} after 3 steps of the first window + 2 budgeted steps per entry of mean_counts; the environment
    is set already."""
    import radnerf_hip as hip
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, SyntheticTrainStream, Trainer
    overrides, _, graphed = ROUTES[name]
    # Trainer's constructor selects rocBLAS for the whole process.  The scene and the stream's frozen render (the target) are built
    # before it and run matrix products: make the selection first, so that the first run of a process sees the library the
    # second one sees (without this the first run's TARGET, not its training, differs from every later run's)
    torch.backends.cuda.preferred_blas_library("cublas")
    torch.manual_seed(0)
    random.seed(0)
    np.random.seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", smooth_lips=False, **overrides))
    stream = SyntheticTrainStream(scene, n_rays=1024, seed=4)
    trainer = (GraphedTrainer if graphed else Trainer)(scene.model, scene.opt, update_extra_interval=0)
    calls = []
    hip.set_timer(hip.KernelTimer(lambda entry, args: calls.append(entry)))     # returns None: nothing is timed, every entry is named
    try:
        for _ in range(3):
            trainer.step(stream.batch())
        for count in mean_counts:
            scene.model.mean_count = count
            for _ in range(2):
                loss = trainer.step(stream.batch())
    finally:
        hip.set_timer(None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    # the ordered entries ran in every step that was enqueued, and no entry that sums with float atomics did
    enqueued = 3 + (len(set(mean_counts)) if graphed else 2 * len(mean_counts))
    assert calls.count("rn_grid_scatter_ordered") == enqueued, calls
    assert not {"rn_grid_scatter_jobs", "rn_grid_scatter_lbc", "rn_grid_scatter_binned", "rn_grid_encode_backward",
                "rn_audio_encode_windows_backward", "rn_audio_encode_windows_backward_acts"} & set(calls), sorted(set(calls))
    if not overrides["torso"]:
        assert calls.count("rn_audio_encode_windows_backward_ordered") == enqueued, calls
    if graphed:
        assert trainer.captures == len(set(mean_counts)) and trainer.replays == 2 * len(mean_counts)
        _RUNS["capture_log"] = list(trainer.capture_log)
    m = scene.model
    out = {"loss": loss.detach().reshape(1)}
    for pname, p in m.named_parameters():
        out["param." + pname] = p.detach()
        st = trainer.optimizer.state.get(p, {})
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st:
                out[key + "." + pname] = st[key]
    tables = ["torso_encoder.embeddings"] if overrides["torso"] else ["encoder.embeddings", "encoder_ambient.embeddings"]
    params = dict(m.named_parameters())
    for t in tables:
        assert params[t].grad is not None, t
        out["grad." + t] = params[t].grad
    assert any(k.startswith("exp_avg.") for k in out)
    return {k: v.detach().cpu().numpy().reshape(-1).view(np.uint32).copy() for k, v in out.items()}


def _first_difference(a, b):
    assert list(a) == list(b)
    for k in a:
        if not np.array_equal(a[k], b[k]):
            return k, int((a[k] != b[k]).sum()), a[k].size
    return None


@pytest.mark.parametrize("name", list(ROUTES))
def test_two_runs_from_the_same_seeds_give_the_same_bits(hiplib, monkeypatch, name):
    _set_environment(ROUTES[name][1], monkeypatch)
    first, second = _run(name), _run(name)
    _RUNS[name] = first
    trained = sum(1 for k in first if k.startswith("exp_avg.") and first[k].any())
    print(name, len(first), "arrays,", trained, "parameters with a gradient; first difference:", _first_difference(first, second))
    assert trained >= 4
    assert any(first[k].any() for k in first if k.startswith("grad."))
    assert _first_difference(first, second) is None
    if name == "graph_head":
        # recorded, not required: does the replayed step compute the eager step's bits?
        eager = _RUNS["head"] if "head" in _RUNS else _run("head")
        print("eager against captured, first difference:", _first_difference(eager, first))


def test_a_graph_captured_before_the_workspace_grew_still_replays(hiplib, monkeypatch):
    """GraphedTrainer keeps its graphs per row capacity and replays an earlier one when the budget comes back.  Budgets either side
    of 65 536 rows: capacity 65 536 (the ordered sum's workspace at 65 536 rows), then 69 632 (a larger workspace replaces it),
    then 65 536 again -- the first graph, which holds the FIRST workspace's address.  That buffer must still be the library's:
    it is kept (radnerf_hip._REPLACED), and the run equals the eager trainer's bit for bit."""
    import radnerf_hip as hip
    _set_environment({}, monkeypatch)
    counts = (60500, 66000, 60500)
    kept = len(hip._REPLACED)
    graphed = _run("graph_head", counts)
    assert [c for _, _, c in _RUNS["capture_log"]] == [65536, 69632]
    assert len(hip._REPLACED) >= kept + 1 and all(b.numel() > 0 for b in hip._REPLACED)
    eager = _run("head", counts)
    # every parameter, every Adam moment and the loss.  Not `.grad`: after a replay of the FIRST graph the parameters' .grad
    # attributes still name the tensors of the graph captured last, which hold the gradients of ITS last replay -- the update
    # inside a graph reads the graph's own gradient tensors, and the moments compared here are made of them
    eager, graphed = [{k: v for k, v in run.items() if not k.startswith("grad.")} for run in (eager, graphed)]
    print("eager against captured over three capacities, first difference:", _first_difference(eager, graphed))
    assert len(eager) > 100 and _first_difference(eager, graphed) is None


def test_a_value_outside_0_and_1_is_an_error(hiplib, monkeypatch):
    from radnerf import train_head
    monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", "yes")
    with pytest.raises(ValueError, match="RN_TRAIN_DETERMINISTIC"):
        train_head.deterministic()
