"""Every route through a training step launches what the recorded commit launched: the ordered C-ABI entry points that pass
through radnerf_hip.call and the number of device activities the profiler sees, per route, against tests/step_routes.json.

The scene is the smallest the training tests use (64x64, 1024 rays, update_extra_interval=0; mean_count set as
test_gpu_train_head.py::test_training_step_launch_count sets it, so that the budgeted step runs).  An eager route takes three
steps of the first window and one budgeted step, then the next step is recorded.  A GraphedTrainer route takes the three steps,
then the names are those of the step that captures and the activities those of the replay after it.

`python tests/test_gpu_step_routes.py --record [FILE] [--parent HASH]` writes the file from the tree it runs in; the committed
one was recorded on the commit its header names, before the routing code was rewritten."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = os.path.join(HERE, "step_routes.json")

HEAD, CAMERA, TORSO = dict(torso=False), dict(torso=False, train_camera=True), dict(torso=True)
# name -> (default_opt overrides, environment, GraphedTrainer?)
ROUTES = {
    "head": (HEAD, {}, False),
    "head_ops": (HEAD, {"RN_TRAIN_HEAD": "ops", "RN_TRAIN_LOSS": "torch"}, False),
    "head_ops_torch": (HEAD, {"RN_TRAIN_HEAD": "ops", "RN_TRAIN_LOSS": "torch", "RN_TRAIN_GLUE": "torch", "RN_MLP_TRAIN": "torch"}, False),
    "march_ops": (HEAD, {"RN_TRAIN_MARCH": "ops"}, False),
    "overlap_off": (HEAD, {"RN_TRAIN_OVERLAP": "0"}, False),
    "scatter_binned": (HEAD, {"RN_SCATTER": "binned"}, False),
    "camera": (CAMERA, {}, False),
    "camera_fused": (CAMERA, {"RN_TRAIN_CAMERA": "fused"}, False),
    "torso": (TORSO, {}, False),
    "torso_fused": (TORSO, {"RN_TORSO_TRAIN": "fused"}, False),
    "torso_fused_host": (TORSO, {"RN_TORSO_TRAIN": "fused", "RN_TORSO_STEP": "host"}, False),
    "graph_head": (HEAD, {}, True),
    "graph_camera_fused": (CAMERA, {"RN_TRAIN_CAMERA": "fused"}, True),
    "graph_torso_fused": (TORSO, {"RN_TORSO_TRAIN": "fused"}, True),
}


def _set_environment(env, setenv, delenv):
    """Only the route's switches are set: every other RN_* variable of the caller's environment goes (the product's defaults)."""
    for name in [n for n in os.environ if n.startswith("RN_")]:
        delenv(name)
    for name, value in env.items():
        setenv(name, value)


def _device_activities(prof):
    return [e.name for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()]


def run_route(name):
    """-> {"calls": [entry points in call order], "activities": device activities of one step}; the environment is set already."""
    import random

    import torch
    from torch.profiler import ProfilerActivity, profile

    import radnerf_hip as hip
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import GraphedTrainer, SyntheticTrainStream, Trainer
    overrides, _, graphed = ROUTES[name]
    torch.manual_seed(0)
    random.seed(0)
    scene = SyntheticScene(H=64, W=64, n_frames=8, device="cuda", opt=default_opt(engine="ops", smooth_lips=False, **overrides))
    stream = SyntheticTrainStream(scene, n_rays=1024, seed=4)
    trainer = (GraphedTrainer if graphed else Trainer)(scene.model, scene.opt, update_extra_interval=0)
    for _ in range(3):
        trainer.step(stream.batch())
    scene.model.mean_count = 12000                           # as after the first 16 steps: the budgeted step
    calls = []
    timer = hip.KernelTimer(lambda entry, args: calls.append(entry))      # returns None: nothing is timed
    if graphed:
        batch = stream.batch()
        hip.set_timer(timer)
        try:
            trainer.step(batch)                              # the capture, and its first replay
        finally:
            hip.set_timer(None)
        assert trainer.captures == 1
    else:
        trainer.step(stream.batch())
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        batch = stream.batch()
        if not graphed:
            hip.set_timer(timer)
        try:
            loss = trainer.step(batch)
        finally:
            hip.set_timer(None)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
    if graphed:
        assert trainer.captures == 1 and trainer.replays == 2
    return {"calls": calls, "activities": len(_device_activities(prof))}


@pytest.fixture(scope="module")
def recorded():
    with open(RECORDED) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(ROUTES))
def test_route_launches_what_the_recorded_commit_launched(hiplib, monkeypatch, recorded, name):
    want = recorded["routes"][name]
    _set_environment(ROUTES[name][1], monkeypatch.setenv, monkeypatch.delenv)
    got = run_route(name)
    print(name, got["activities"], "device activities,", len(got["calls"]), "entry points:", got["calls"])
    if "calls" in want:
        assert got["calls"] == want["calls"]
    if "activities" in want:
        assert got["activities"] == want["activities"]
    assert "calls" in want or "activities" in want, name


def _record(path, parent):
    for p in (os.path.join(os.path.dirname(HERE), "rad-nerf_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    if parent is None:
        parent = subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True, check=True).stdout.strip()
    routes = {}
    for name, (_, env, _) in ROUTES.items():
        _set_environment(env, os.environ.__setitem__, os.environ.__delitem__)
        routes[name] = run_route(name)
        print(name, routes[name]["activities"], len(routes[name]["calls"]), flush=True)
        with open(path, "w") as f:                           # after every route: a run that stops early leaves what it had
            json.dump({"recorded_on_commit": parent, "routes": routes}, f, indent=1)
            f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    argv = sys.argv[1:]
    if not argv or argv[0] != "--record":
        sys.exit("usage: test_gpu_step_routes.py --record [FILE] [--parent HASH]")
    parent = argv[argv.index("--parent") + 1] if "--parent" in argv else None
    rest = [a for i, a in enumerate(argv[1:], 1) if a != "--parent" and argv[i - 1] != "--parent"]
    _record(rest[0] if rest else RECORDED, parent)
