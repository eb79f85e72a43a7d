"""radnerf.cli end to end on tests/dataset_dir.py's 20 x 16 directory: train two epochs, continue for a third, render a clip from
the checkpoint.  One module-scoped run of each stage; the tests read what it left."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_dir as dd  # noqa: E402


@pytest.fixture(scope="module")
def runs(tmp_path_factory, hiplib):
    from radnerf import cli
    root = str(tmp_path_factory.mktemp("dataset"))
    ws = str(tmp_path_factory.mktemp("workspace"))
    dd.write_dataset(root, 0)
    lines = []
    log = lambda *a: lines.append(" ".join(str(x) for x in a))
    base = [root, "--workspace", ws, "--num_rays", "256", "-O"]
    first = cli.main(base + ["--iters", "48"], log=log, decode=dd.npy_decode)
    first_ckpt = {k: v for k, v in torch.load(first["checkpoints"][-1], map_location="cpu", weights_only=False).items()}
    second = cli.main(base + ["--iters", "72", "--ckpt", "latest"], log=log, decode=dd.npy_decode)
    test = cli.main(base + ["--test", "--pose", os.path.join(root, "clip.json"), "--aud", os.path.join(root, "clip_aud.npy")], log=log,
                    decode=dd.npy_decode)
    return dict(root=root, ws=ws, first=first, first_ckpt=first_ckpt, second=second, test=test, lines=lines)


def test_training_runs_two_epochs_and_evaluates(runs):
    first = runs["first"]
    assert first["epoch"] == 2 and first["global_step"] == 48 and first["first_epoch"] == 1
    assert len(first["losses"]) == 48 and all(np.isfinite(first["losses"]))
    assert [os.path.basename(p) for p in first["checkpoints"]] == ["ngp_ep0001.pth", "ngp_ep0002.pth"]
    assert len(first["evals"]) == 1                                 # eval_interval = 208 epochs: only the closing test evaluation
    epoch, res = first["evals"][0]
    assert epoch == 2 and np.isfinite(res["loss"]) and np.isfinite(res["psnr"]) and len(res["per_frame"]) == dd.N_VAL
    video = np.load(first["video"])
    assert video.dtype == np.uint8 and video.shape == (dd.N_VAL, dd.H, dd.W, 3)         # without --pose: the val split replayed
    assert np.load(first["video"].replace(".npy", "_depth.npy")).shape == (dd.N_VAL, dd.H, dd.W)
    assert any("arithmetic follows the RN_* switches" in ln for ln in runs["lines"])


def test_the_checkpoint_is_a_full_one(runs):
    from radnerf import cli
    from radnerf.checkpoint import load_checkpoint
    from radnerf.network import NeRFNetwork
    ck = runs["first_ckpt"]
    assert ck["global_step"] == 48 and ck["epoch"] == 2
    assert ck["ema"] is not None and len(ck["ema"]["shadow_params"]) > 0 and ck["ema"]["decay"] == 0.95
    steps = {int(st["step"]) for st in ck["optimizer"]["state"].values()}
    assert steps == {48} and len(ck["optimizer"]["param_groups"]) >= 2
    fresh = NeRFNetwork(cli.parse([runs["root"], "-O"]))
    missing, unexpected = load_checkpoint(fresh, dict(ck))
    assert missing == [] and unexpected == []
    assert fresh.checkpoint_meta["global_step"] == 48


def test_continuing_from_latest(runs):
    second = runs["second"]
    assert second["first_epoch"] == 3 and second["start_step"] == 48 and second["epoch"] == 3 and second["global_step"] == 72
    assert len(second["losses"]) == 24 and all(np.isfinite(second["losses"]))
    want = [lr0 * 0.1 ** (48 / 72) for lr0 in sorted({5e-3, 5e-4, 5 * 5e-4})]      # tables, networks, the attention net (get_params)
    got = sorted(set(second["start_lr"]))                       # a host mirror in double: the same expression, a few ulps at most
    assert len(got) == 3 and np.allclose(got, want, rtol=1e-12, atol=0)
    ck = torch.load(second["checkpoints"][-1], map_location="cpu", weights_only=False)
    assert {int(st["step"]) for st in ck["optimizer"]["state"].values()} == {72} and ck["global_step"] == 72
    assert os.path.basename(second["checkpoints"][-1]) == "ngp_ep0003.pth"


def test_captured_training_replays_graphs(runs, tmp_path):
    """--captured: the same run through GraphedTrainer -- the first window eager, the rest replayed."""
    from radnerf import cli
    from radnerf.train import GraphedTrainer
    done = cli.main([runs["root"], "--workspace", str(tmp_path), "--num_rays", "256", "-O", "--iters", "48", "--captured", "--ckpt", "scratch"],
                    log=lambda *a: None, decode=dd.npy_decode)
    tr = done["trainer"]
    assert isinstance(tr, GraphedTrainer) and tr.captures >= 1 and tr.replays >= 16 and tr.global_step == 48
    assert len(done["losses"]) == 48 and all(np.isfinite(done["losses"]))
    ck = torch.load(done["checkpoints"][-1], map_location="cpu", weights_only=False)
    assert {int(st["step"]) for st in ck["optimizer"]["state"].values()} == {48} and ck["ema"] is not None


def test_lip_fine_tuning_from_the_command_line(tmp_path):
    """--finetune_lips --lpips_weights: one epoch of the rect / pixel alternation with the perceptual term, on the directory at
    8 x the size (160 x 128: every lips rect is at least 34 pixels wide, the perceptual network's smallest image is 31)."""
    import percepref64 as R
    from radnerf import cli
    from radnerf.percep import LAYERS, _LPIPS_SLICES
    root, ws = str(tmp_path / "data"), str(tmp_path / "ws")
    dd.write_dataset(root, 0, scale=8)
    weights, biases, lins, _ = R.seeded_weights()
    sd = {}
    for l, prefix in enumerate(_LPIPS_SLICES):
        sd[f"{prefix}.weight"], sd[f"{prefix}.bias"], sd[f"lin{l}.model.1.weight"] = weights[l], biases[l], lins[l]
    assert len(sd) == 3 * len(LAYERS)
    torch.save(sd, str(tmp_path / "alex.pth"))
    done = cli.main([root, "--workspace", ws, "--num_rays", "256", "-O", "--iters", "24", "--ckpt", "scratch", "--finetune_lips",
                     "--lpips_weights", str(tmp_path / "alex.pth")], log=lambda *a: None, decode=dd.npy_decode)
    tr = done["trainer"]
    assert tr.patch_criterion is not None and tr.lr_gamma == 0.05 and tr.update_extra_interval == int(1e9) and tr.global_step == 24
    assert len(done["losses"]) == 24 and all(np.isfinite(done["losses"]))
    # even steps carry the perceptual term on top of the pixel loss: on these random frames it is the larger part
    assert np.mean(done["losses"][0::2]) != np.mean(done["losses"][1::2])
    assert np.load(done["video"]).shape == (dd.N_VAL, 8 * dd.H, 8 * dd.W, 3)


def test_torso_stage_freezes_the_loaded_head(runs, tmp_path):
    """--torso --head_ckpt: the head's parameters come from the checkpoint, stay frozen and unchanged; the torso's train."""
    from radnerf import cli
    head = runs["first_ckpt"]["model"]
    done = cli.main([runs["root"], "--workspace", str(tmp_path), "--num_rays", "256", "-O", "--iters", "24", "--ckpt", "scratch", "--torso",
                     "--head_ckpt", runs["first"]["checkpoints"][-1]], log=lambda *a: None, decode=dd.npy_decode)
    params = dict(done["trainer"].model.named_parameters())
    frozen = [k for k, v in params.items() if not v.requires_grad]
    trainable = [k for k, v in params.items() if v.requires_grad]
    assert frozen and trainable and all(k in head for k in frozen) and not any(k in head for k in trainable)
    assert all("torso" in k for k in trainable) and "sigma_net.net.0.weight" in frozen
    assert all(torch.equal(params[k].detach().cpu(), head[k]) for k in frozen)
    assert len(done["losses"]) == 24 and all(np.isfinite(done["losses"])) and done["global_step"] == 24


def test_rendering_a_clip_from_the_checkpoint(runs):
    """--test --pose --aud writes uint8 [30,20,16,3]: bit-equal to the same checkpoint rendered through ClipScene directly."""
    from radnerf import cli
    from radnerf.checkpoint import load_checkpoint
    from radnerf.clip import ClipScene
    from radnerf.network import NeRFNetwork
    test = runs["test"]
    video = np.load(test["video"])
    assert video.dtype == np.uint8 and video.shape == (dd.N_AUD, dd.H, dd.W, 3) and test["epoch"] == 3
    assert test["evals"] == []                                          # a driving audio file: no ground truth
    opt = test["opt"]
    assert opt.smooth_path and opt.smooth_eye and opt.smooth_lips
    model = NeRFNetwork(opt).cuda()
    load_checkpoint(model, cli.latest_checkpoint(runs["ws"]), map_location="cuda")
    scene = ClipScene.from_files(model, opt, "cuda", decode=dd.npy_decode)
    with torch.no_grad():
        model.enc_a = None
        want = torch.stack([scene.render(i, want_u8=True)["image_u8"].reshape(dd.H, dd.W, 3).clone() for i in range(scene.n_frames)])
    assert np.array_equal(video, want.cpu().numpy())
    assert len(glob.glob(os.path.join(runs["ws"], "results", "*.npy"))) >= 3
