"""radnerf/cli.py without a GPU: parse (the reference's implied settings, the refused flags) and plan (epochs, evaluation cadence,
LR decay)."""
import types

import pytest

from radnerf import cli


def test_defaults_are_the_reference_cli(tmp_path):
    opt = cli.parse(["data/obama"])
    assert opt.path == "data/obama" and opt.workspace == "workspace" and opt.ckpt == "latest"
    assert (opt.iters, opt.lr, opt.lr_net, opt.num_rays, opt.max_steps, opt.update_extra_interval) == (200000, 5e-3, 5e-4, 65536, 16, 16)
    assert (opt.bound, opt.scale, opt.offset, opt.dt_gamma, opt.min_near) == (1, 4, [0, 0, 0], 1 / 256, 0.05)
    assert (opt.density_thresh, opt.density_thresh_torso, opt.torso_shrink, opt.patch_size) == (10, 0.01, 0.8, 1)
    assert (opt.att, opt.ind_dim, opt.ind_num, opt.ind_dim_torso, opt.smooth_path_window, opt.fix_eye) == (2, 4, 10000, 8, 7, -1)
    assert (opt.data_range, opt.bg_img, opt.aud, opt.preload, opt.lambda_amb) == ([0, -1], "", "", 0, 0.1)
    assert "esperanto" in opt.asr_model and opt.cuda_ray is True
    for flag in ("fp16", "exp_eye", "smooth_path", "smooth_eye", "smooth_lips", "torso", "finetune_lips", "part", "part2", "test",
                 "test_train", "emb", "asr", "train_camera", "captured", "png"):
        assert getattr(opt, flag) is False, flag


def test_O_test_and_finetune_lips_imply_their_settings(tmp_path):
    opt = cli.parse(["d", "-O"])
    assert opt.fp16 and opt.exp_eye and not opt.smooth_path
    opt = cli.parse(["d", "--test", "--pose", "p.json", "--aud", "a.npy"])
    assert opt.smooth_path and opt.smooth_eye and opt.smooth_lips and not opt.exp_eye and (opt.pose, opt.aud) == ("p.json", "a.npy")
    weights = tmp_path / "alex.pth"
    weights.write_bytes(b"")
    opt = cli.parse(["d", "--finetune_lips", "--lpips_weights", str(weights)])
    assert opt.finetune_lips and opt.update_extra_interval == int(1e9)
    assert cli.parse(["d", "--preload", "2"]).preload == 2                 # accepted, ignored


@pytest.mark.parametrize("flag", ["--gui", "--asr", "--asr_wav=x.wav", "--asr_play", "--asr_save_feats", "--emb"])
def test_refused_flags_say_they_are_not_built(flag, capsys):
    with pytest.raises(SystemExit) as e:
        cli.parse(["d", flag])
    assert e.value.code == 2
    assert "not built here" in capsys.readouterr().err


def test_lips_without_weights_ends_before_any_gpu_call(capsys, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: pytest.fail("a GPU call was made"))
    for argv in (["d", "--finetune_lips"], ["d", "--patch_size", "32"]):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2
        assert "--lpips_weights" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(["d", "--finetune_lips", "--lpips_weights", "/nonexistent/alex.pth"])
    assert "is not a file" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse(["d", "--patch_size", "32", "--num_rays", "1000", "--lpips_weights", "x"])


def test_plan_for_24_frames_and_50_iters(tmp_path):
    p = cli.plan(cli.parse(["d", "--iters", "50"]), 24)
    assert (p["epochs"], p["eval_interval"], p["lr_gamma"], p["ema_decay"], p["iters"], p["update_extra_interval"]) == (3, 208, 0.1, 0.95, 50, 16)
    weights = tmp_path / "alex.pth"
    weights.write_bytes(b"")
    p = cli.plan(cli.parse(["d", "--iters", "50", "--finetune_lips", "--lpips_weights", str(weights)]), 24)
    assert (p["epochs"], p["lr_gamma"], p["update_extra_interval"]) == (3, 0.05, int(1e9))
    assert cli.plan(types.SimpleNamespace(iters=200000, finetune_lips=False, update_extra_interval=16), 6000)["eval_interval"] == 1
    assert cli.plan(cli.parse(["d", "--iters", "48"]), 24)["epochs"] == 2
    with pytest.raises(ValueError):
        cli.plan(cli.parse(["d"]), 0)


def test_checkpoint_names(tmp_path):
    assert cli.checkpoint_path("ws", 7).replace("\\", "/") == "ws/checkpoints/ngp_ep0007.pth"
    assert cli.latest_checkpoint(str(tmp_path)) is None
    (tmp_path / "checkpoints").mkdir()
    for e in (2, 10, 9):
        (tmp_path / "checkpoints" / f"ngp_ep{e:04d}.pth").write_bytes(b"")
    assert cli.latest_checkpoint(str(tmp_path)).endswith("ngp_ep0010.pth")
