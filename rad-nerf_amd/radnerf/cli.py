"""`python -m radnerf.cli data/obama --workspace trial -O --iters 200000`: train on a dataset directory, or render a clip from a
checkpoint plus a pose file and an audio-feature file -- the wiring of the reference's main.py:109-247 over this tree's classes.

    train     DeviceTrainSet.from_directory -> Trainer / GraphedTrainer (LR decay and EMA inside the Adam launches) ->
              workspace/checkpoints/ngp_ep%04d.pth every epoch, Trainer.evaluate on the val split every eval_interval epochs
    render    ClipScene + FrameParallelRenderer -> workspace/results/<name>.npy (uint8 [F,H,W,3]) and <name>_depth.npy;
              --video: <name>.avi beside it, Motion-JPEG encoded on the device, --audio_wav laid under it (radnerf/video.py)

parse(argv) -> opt, plan(opt, n_frames) -> the schedule, main(argv) -> a dict of what was done.  parse and plan touch no GPU.

Everything this module adds runs once per run, epoch or frame on the host; per training step it calls DeviceTrainSet's one batch
launch and Trainer.step, per frame ClipScene.render.  Flags keep the reference's names and defaults.  `-O` records fp16 and
exp_eye; fp16 only records: the arithmetic follows the RN_* switches (radnerf/switches.py is their only reader, nothing is set
here).  `--preload` is accepted and ignored (the set is always device-resident uint8).  Not built here, and refused: --gui, --asr*
(live audio: `python -m radnerf.live` renders from an audio stream, radnerf/live.py), --emb, --train_camera from this entry point.  --video writes Motion-JPEG in AVI with PCM audio and nothing else:
no MP4 / H.264, no compressed audio; the .npy stays what any other encoder reads.  --aud_wav FILE --asr_weights FILE drive the
clip from a 16 kHz .wav: its wav2vec2 logits (radnerf/asr.py) go where --aud's would, and with --video the same file is laid
under the frames unless --audio_wav names another.  With --resample, --aud_wav takes any PCM or float .wav at any rate: it is
decoded and resampled to 16 kHz on the device (radnerf/resample.py); a file the AVI writer cannot carry (float samples) goes under
the frames as the resampled signal in PCM16.
Continuing from a checkpoint restores model, optimizer, EMA, epoch and step count; it is NOT bit-identical to an uninterrupted
run, because the occupancy refresh draws from Python's `random`.
"""
import argparse
import copy
import glob
import math
import os
import random
import sys

import numpy as np

REFUSED = {"gui": "the GUI", "asr": "live ASR", "asr_wav": "live ASR", "asr_play": "live ASR", "asr_save_feats": "live ASR",
           "emb": "the --emb route (audio class + embedding)", "train_camera": "camera-pose training from this entry point"}


def _parser():
    p = argparse.ArgumentParser(prog="python -m radnerf.cli", description="RAD-NeRF on HIP: train on a dataset directory, render clips")
    p.add_argument("path", type=str)
    p.add_argument("-O", action="store_true", help="equals --fp16 --cuda_ray --exp_eye")
    p.add_argument("--test", action="store_true", help="test mode (load model and test dataset)")
    p.add_argument("--test_train", action="store_true", help="test mode (load model and train dataset)")
    p.add_argument("--data_range", type=int, nargs="*", default=[0, -1], help="data range to use")
    p.add_argument("--workspace", type=str, default="workspace")
    p.add_argument("--seed", type=int, default=0)
    # training
    p.add_argument("--iters", type=int, default=200000)
    p.add_argument("--lr", type=float, default=5e-3)
    p.add_argument("--lr_net", type=float, default=5e-4)
    p.add_argument("--ckpt", type=str, default="latest", help="latest | scratch | PATH")
    p.add_argument("--num_rays", type=int, default=4096 * 16)
    p.add_argument("--cuda_ray", action="store_true")
    p.add_argument("--max_steps", type=int, default=16)
    p.add_argument("--update_extra_interval", type=int, default=16)
    p.add_argument("--fp16", action="store_true")
    p.add_argument("--lambda_amb", type=float, default=0.1)
    p.add_argument("--bg_img", type=str, default="")
    p.add_argument("--exp_eye", action="store_true")
    p.add_argument("--fix_eye", type=float, default=-1)
    p.add_argument("--smooth_eye", action="store_true")
    p.add_argument("--torso_shrink", type=float, default=0.8)
    # dataset
    p.add_argument("--preload", type=int, default=0, help="accepted and ignored: the set is always device-resident uint8")
    p.add_argument("--bound", type=float, default=1)
    p.add_argument("--scale", type=float, default=4)
    p.add_argument("--offset", type=float, nargs="*", default=[0, 0, 0])
    p.add_argument("--dt_gamma", type=float, default=1 / 256)
    p.add_argument("--min_near", type=float, default=0.05)
    p.add_argument("--density_thresh", type=float, default=10)
    p.add_argument("--density_thresh_torso", type=float, default=0.01)
    p.add_argument("--patch_size", type=int, default=1)
    p.add_argument("--finetune_lips", action="store_true")
    p.add_argument("--smooth_lips", action="store_true")
    p.add_argument("--torso", action="store_true")
    p.add_argument("--head_ckpt", type=str, default="")
    p.add_argument("--radius", type=float, default=3.35)
    p.add_argument("--fovy", type=float, default=21.24)
    p.add_argument("--att", type=int, default=2)
    p.add_argument("--aud", type=str, default="")
    p.add_argument("--ind_dim", type=int, default=4)
    p.add_argument("--ind_num", type=int, default=10000)
    p.add_argument("--ind_dim_torso", type=int, default=8)
    p.add_argument("--part", action="store_true")
    p.add_argument("--part2", action="store_true")
    p.add_argument("--smooth_path", action="store_true")
    p.add_argument("--smooth_path_window", type=int, default=7)
    p.add_argument("--asr_model", type=str, default="cpierse/wav2vec2-large-xlsr-53-esperanto", help="picks the audio-feature file")
    # refused: kept so that the refusal can say what is not built
    for name in REFUSED:
        p.add_argument("--" + name, nargs="?", const=True, default=False, help=argparse.SUPPRESS)
    # this tree's own
    p.add_argument("--pose", type=str, default="", help="transforms file of the clip to render (default: the val split)")
    p.add_argument("--lpips_weights", type=str, default="", help="state dict of lpips.LPIPS(net='alex'); nothing is fetched")
    p.add_argument("--captured", action="store_true", help="replay the training step from captured graphs (GraphedTrainer)")
    p.add_argument("--png", action="store_true", help="also write the frames as PNG files (needs PIL)")
    p.add_argument("--video", action="store_true", help="also write results/<name>.avi: Motion-JPEG encoded on the device")
    p.add_argument("--video_quality", type=int, default=90, help="JPEG quality of --video, 1 .. 100")
    p.add_argument("--video_subsampling", type=str, default="420", choices=("420", "444"))
    p.add_argument("--video_fps", type=float, default=25, help="frame rate of --video (not --fps, the reference's ASR rate)")
    p.add_argument("--audio_wav", type=str, default="", help="PCM .wav to lay under --video")
    p.add_argument("--aud_wav", type=str, default="", help="16 kHz PCM .wav that drives the clip: its wav2vec2 logits replace --aud (radnerf/asr.py)")
    p.add_argument("--resample", action="store_true", help="--aud_wav: take any PCM or float .wav, resampled to 16 kHz on the device")
    p.add_argument("--asr_weights", type=str, default="", help="state dict of Wav2Vec2ForCTC for --aud_wav; nothing is fetched")
    p.add_argument("--asr_config", type=str, default="", help="the model's config.json (default: the large shape)")
    p.add_argument("-l", type=int, default=10, help="--aud_wav: chunks of left context per window")
    p.add_argument("-m", type=int, default=50, help="--aud_wav: chunks a window contributes")
    p.add_argument("-r", type=int, default=10, help="--aud_wav: chunks of right context per window")
    p.add_argument("--name", type=str, default="ngp")
    p.add_argument("--engine", type=str, default="fused", choices=("ops", "fused"))
    return p


def parse(argv=None):
    """argv -> opt with the reference's implied settings (main.py:111-129); errors end through argparse (SystemExit 2)."""
    p = _parser()
    opt = p.parse_args(argv)
    for name, what in REFUSED.items():
        if getattr(opt, name):
            p.error(f"--{name}: {what} is not built here")
    if opt.O:
        opt.fp16 = True
        opt.exp_eye = True
    if opt.test:
        opt.smooth_path = True
        opt.smooth_eye = True
        opt.smooth_lips = True
    opt.cuda_ray = True
    if opt.patch_size > 1 and (opt.num_rays % (opt.patch_size ** 2) != 0 or opt.num_rays < opt.patch_size ** 2):
        p.error("--patch_size: num_rays must be a positive multiple of patch_size ** 2")
    if opt.finetune_lips:
        opt.update_extra_interval = int(1e9)          # no occupancy refresh in the fine-tuning stage
    training = not (opt.test or opt.test_train)
    if training and (opt.finetune_lips or opt.patch_size > 1) and not opt.lpips_weights:
        p.error("--finetune_lips / --patch_size > 1 need --lpips_weights FILE (the state dict of lpips.LPIPS(net='alex')): "
                "the perceptual term's weights are not fetched from anywhere")
    if opt.lpips_weights and not os.path.isfile(opt.lpips_weights):
        p.error(f"--lpips_weights: {opt.lpips_weights} is not a file")
    if opt.iters <= 0:
        p.error("--iters must be positive")
    if not 1 <= opt.video_quality <= 100:
        p.error("--video_quality is 1 .. 100")
    if not opt.video_fps > 0:
        p.error("--video_fps must be positive")
    if opt.audio_wav:
        from radnerf.video import check_wav
        try:
            check_wav(opt.audio_wav)
        except ValueError as e:
            p.error(f"--audio_wav: {e}")
    if opt.aud_wav:
        if opt.aud:
            p.error("--aud_wav and --aud both name the clip's audio features; give one")
        if not opt.asr_weights:
            p.error("--aud_wav needs --asr_weights FILE (the state dict of Wav2Vec2ForCTC): the model's weights are not fetched from anywhere")
        for flag in ("aud_wav", "asr_weights", "asr_config"):
            if getattr(opt, flag) and not os.path.isfile(getattr(opt, flag)):
                p.error(f"--{flag}: {getattr(opt, flag)} is not a file")
        if opt.l < 0 or opt.r < 0 or opt.m < 1:
            p.error("-l and -r must not be negative, -m must be positive")
        try:
            if opt.resample:
                from radnerf import resample
                resample.plan(resample.check_audio(opt.aud_wav)[0])
            else:
                from radnerf.asr import check_wav as check_wav16k
                check_wav16k(opt.aud_wav)
        except ValueError as e:
            p.error(f"--aud_wav: {e}")
    elif opt.asr_weights or opt.asr_config:
        p.error("--asr_weights / --asr_config go with --aud_wav FILE")
    opt.test_train = bool(opt.test_train)
    return opt


def plan(opt, n_frames):
    """The schedule of a training run over n_frames frames (main.py:216-233): epochs, evaluation cadence, LR decay, EMA."""
    n_frames = int(n_frames)
    if n_frames < 1:
        raise ValueError("plan: no frames")
    return dict(epochs=int(math.ceil(opt.iters / n_frames)), eval_interval=max(1, int(5000 / n_frames)),
                lr_gamma=0.05 if opt.finetune_lips else 0.1, ema_decay=0.95, iters=int(opt.iters),
                update_extra_interval=int(opt.update_extra_interval), steps_per_epoch=n_frames)


# ------------------------------------------------------------------------------------------------------------ pieces
def checkpoint_path(workspace, epoch, name="ngp"):
    return os.path.join(workspace, "checkpoints", f"{name}_ep{epoch:04d}.pth")


def latest_checkpoint(workspace, name="ngp"):
    found = sorted(glob.glob(os.path.join(workspace, "checkpoints", f"{name}_ep*.pth")))
    return found[-1] if found else None


def _which_checkpoint(opt, log):
    if opt.ckpt == "scratch":
        return None
    if opt.ckpt == "latest":
        path = latest_checkpoint(opt.workspace, opt.name)
        if path is None:
            log("[WARN] no checkpoint found, the model starts from its initialisation")
        return path
    if not os.path.isfile(opt.ckpt):
        raise FileNotFoundError(f"--ckpt: {opt.ckpt} is not a file")
    return opt.ckpt


def _distributed():
    """(rank, world, dist or None): the ranks of torch.distributed.run when launched under it (torch's own test; this module reads
    nothing from the process environment).  One node: rank r takes GPU r."""
    import torch
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_torchelastic_launched()):
        return 0, 1, None
    if not dist.is_initialized():
        dist.init_process_group("nccl")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(rank % torch.cuda.device_count())
    return (rank, world, dist) if world > 1 else (0, 1, None)


def _model(opt, device, log):
    import torch
    from radnerf.network import NeRFNetwork
    model = NeRFNetwork(opt)
    if opt.torso and opt.head_ckpt != "":                         # main.py:142-157: the head, loaded non-strictly and frozen
        head = torch.load(opt.head_ckpt, map_location="cpu", weights_only=False)["model"]
        missing, unexpected = model.load_state_dict(head, strict=False)
        if missing:
            log(f"[WARN] missing keys: {missing}")
        if unexpected:
            log(f"[WARN] unexpected keys: {unexpected}")
        for k, v in model.named_parameters():
            if k in head:
                v.requires_grad = False
    return model.to(device)


def clip_of_split(d):
    """A LoadedSplit as the clip the reference's `test` loader replays (NeRFDataset(type='test').dataloader())."""
    from radnerf.datafiles import LoadedClip
    return LoadedClip(H=d.H, W=d.W, poses=d.poses, intrinsics=d.intrinsics, auds=d.auds, eye_area=d.eye_area, bg=d.bg)


def render_clip(opt, model, device, out_dir, name, log=print, decode=None):
    """The clip through ClipScene + FrameParallelRenderer (one rank, or the ranks of torch.distributed.run) ->
    <out_dir>/<name>.npy uint8 [F,H,W,3] and, on one rank, <name>_depth.npy float32 [F,H,W]; --png: the frames as PNG files;
    --video: <name>.avi (one rank: every frame goes to the VideoSink as it is rendered; several: rank 0 encodes the gathered stack).
    The lip-smoothing state starts fresh.  -> (path of the frames, n_frames); the path is None off rank 0."""
    import torch
    from radnerf.clip import ClipScene
    from radnerf.datafiles import load_clip, load_split
    from radnerf.parallel import FrameParallelRenderer
    if opt.pose:
        clip = load_clip(opt, decode=decode)
    else:
        clip = clip_of_split(load_split(opt.path, opt, "train" if opt.test_train else "test", decode=decode))
    scene = ClipScene(model, clip, opt, device)
    rank, world, dist = _distributed()
    renderer = FrameParallelRenderer(scene, rank=rank, world=world, dist=dist, gather_to="rank0")
    n = scene.n_frames
    steps = -(-n // world)
    model.enc_a = None
    frames, depths = [], []
    sink = _video_sink(opt, scene.H, scene.W, device, out_dir, name) if opt.video and rank == 0 else None
    with torch.no_grad():
        for s in range(steps):
            u8 = renderer.step(s)
            if world == 1:
                frames.append(u8.clone())
                if sink is not None:
                    sink.push(frames[-1])
                depths.append(scene.last_out["depth"].reshape(scene.H, scene.W).float().clone())
        done = renderer.finish()
    if world > 1:
        if rank != 0:
            return None, n
        video = torch.stack([f for stack in done for f in stack.unbind(0)])[:n]
        if sink is not None:
            for f in video.to(device).unbind(0):
                sink.push(f)
        video = video.cpu().numpy()
    else:
        video = torch.stack(frames).cpu().numpy()
    if sink is not None:
        log(f"[INFO] wrote {sink.finish()}: {sink.files} frames at {opt.video_fps:g} per second")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, name + ".npy")
    np.save(path, video)
    if depths:
        np.save(os.path.join(out_dir, name + "_depth.npy"), torch.stack(depths).cpu().numpy())
    if opt.png:
        from PIL import Image
        for i, frame in enumerate(video):
            Image.fromarray(frame).save(os.path.join(out_dir, f"{name}_{i:04d}.png"))
    log(f"[INFO] wrote {path}: {video.shape[0]} frames of {video.shape[1]} x {video.shape[2]}")
    return path, n


def avi_path(out_dir, name):
    return os.path.join(out_dir, name + ".avi")


def _video_sink(opt, H, W, device, out_dir, name):
    from radnerf.video import AviWriter, JpegEncoder, VideoSink
    os.makedirs(out_dir, exist_ok=True)
    writer = AviWriter(avi_path(out_dir, name), H, W, opt.video_fps, audio=opt.audio_wav or getattr(opt, "audio_track", None) or opt.aud_wav or None)
    return VideoSink(writer, JpegEncoder(H, W, opt.video_quality, opt.video_subsampling), batch=8, device=device)


def resampled_track(path, samples, log=print):
    """--video with --resample: None when the AVI writer can carry `path` itself (integer PCM at any rate), else the resampled
    signal as (rate, channels, bytes per sample, PCM16 bytes), with one [INFO] line.  samples: the 16 kHz signal, or a callable
    that gives it (asked only when the track is needed)."""
    from radnerf.resample import pcm16_track
    from radnerf.video import check_wav
    try:
        check_wav(path)
        return None
    except ValueError:
        log(f"[INFO] {path}: the video's audio track is the resampled signal, 16 kHz mono PCM16 (the AVI writer takes what the `wave` module reads as PCM)")
        return pcm16_track(samples() if callable(samples) else samples)


def wav_features(opt, model, device, log=print):
    """--aud_wav: the wav2vec2 logits of the file as [F,C,16] on the device, left at opt.aud_features where datafiles' loaders take
    the clip's audio from (in opt.aud's place).  The logit width must be the audio net's input width."""
    from radnerf.asr import Wav2Vec2CTC, read_wav
    from radnerf.resample import samples_16k
    asr = Wav2Vec2CTC.from_files(opt.asr_weights, opt.asr_config or None)
    want = int(model.audio_in_dim)
    if asr.vocab_size != want:
        raise ValueError(f"--aud_wav: the model of --asr_weights gives logits of width {asr.vocab_size}, the audio net of this checkpoint "
                         f"takes {want} (--asr_model picks it)")
    samples = samples_16k(opt.aud_wav, device) if opt.resample else read_wav(opt.aud_wav)
    feats = asr.to(device).features_from_samples(samples, opt.l, opt.m, opt.r, layout="FC16")
    if opt.resample and opt.video and not opt.audio_wav:
        opt.audio_track = resampled_track(opt.aud_wav, samples, log)
    log(f"[INFO] {opt.aud_wav}: {feats.shape[0]} audio frames of width {feats.shape[1]}")
    opt.aud_features = feats
    return feats


def _perceptual(opt, device):
    if not opt.lpips_weights:
        return None
    import torch
    from radnerf.percep import PerceptualAlex
    return PerceptualAlex.from_lpips_state_dict(torch.load(opt.lpips_weights, map_location="cpu", weights_only=False)).to(device)


def _evaluate(trainer, split_set, log, what):
    res = trainer.evaluate(split_set, range(split_set.F))
    log(f"[INFO] {what}: loss {res['loss']:.6f}, PSNR {res['psnr']:.3f} over {split_set.F} frames")
    return res


def _val_set(opt, device, split, decode=None):
    from radnerf.dataset import DeviceTrainSet
    o = copy.copy(opt)
    o.finetune_lips = False                    # evaluation samples whole frames; no lips rect is needed (or checked)
    return DeviceTrainSet.from_directory(opt.path, o, split, num_rays=opt.num_rays, seed=opt.seed, device=device, decode=decode)


# -------------------------------------------------------------------------------------------------------------- main
def main(argv=None, log=print, decode=None):
    """decode: another image decoder for every file this run reads (datafiles.py), e.g. a test's."""
    opt = parse(argv)
    log(opt)
    log(f"[INFO] fp16 = {opt.fp16}: recorded only -- arithmetic follows the RN_* switches")
    import torch
    from radnerf.checkpoint import load_checkpoint, save_checkpoint
    from radnerf.dataset import DeviceTrainSet
    from radnerf.train import GraphedTrainer, Trainer, lips_schedule
    if not torch.cuda.is_available():
        raise RuntimeError("radnerf.cli needs a GPU")
    random.seed(opt.seed)
    np.random.seed(opt.seed)
    torch.manual_seed(opt.seed)
    rank, world, _ = _distributed()
    device = torch.device("cuda", torch.cuda.current_device())
    model = _model(opt, device, log)
    results_dir = os.path.join(opt.workspace, "results")
    done = dict(opt=opt, losses=[], evals=[], checkpoints=[], video=None, avi=None)

    if opt.test or opt.test_train:
        path = _which_checkpoint(opt, log)
        if path is None:
            raise FileNotFoundError("--test needs a checkpoint (--ckpt latest found none)")
        missing, unexpected = load_checkpoint(model, path, map_location=device)
        log(f"[INFO] loaded {path}" + (f", missing {missing}" if missing else "") + (f", unexpected {unexpected}" if unexpected else ""))
        epoch = int(getattr(model, "checkpoint_meta", {}).get("epoch", 0))
        done.update(epoch=epoch, global_step=int(getattr(model, "checkpoint_meta", {}).get("global_step", 0)))
        if opt.aud_wav:
            wav_features(opt, model, device, log)
        if not opt.pose and opt.aud == "" and not opt.aud_wav and rank == 0:           # has_gt: the set's own frames and audio
            split = _val_set(opt, device, "train" if opt.test_train else "test", decode)
            split.install(model)
            done["evals"].append((epoch, _evaluate(Trainer(model, opt, iters=opt.iters), split, log, "test")))
            del split
        done["video"], done["n_frames"] = render_clip(opt, model, device, results_dir, f"{opt.name}_ep{epoch:04d}", log, decode)
        done["avi"] = avi_path(results_dir, f"{opt.name}_ep{epoch:04d}") if opt.video and done["video"] else None
        return done

    if world > 1:
        raise RuntimeError("training runs on one GPU; launch only --test under torch.distributed.run")
    ds = DeviceTrainSet.from_directory(opt.path, opt, "train", num_rays=opt.num_rays, seed=opt.seed, device=device, decode=decode)
    assert ds.F < opt.ind_num, f"[ERROR] dataset too many frames: {ds.F}, please increase --ind_num to this number!"
    ds.install(model)
    p = plan(opt, ds.F)
    log(f"[INFO] {ds.F} frames of {ds.H} x {ds.W}, max_epoch = {p['epochs']}, eval every {p['eval_interval']} epochs")
    kw = dict(lr=opt.lr, lr_net=opt.lr_net, update_extra_interval=p["update_extra_interval"], iters=p["iters"], lambda_amb=opt.lambda_amb,
              patch_criterion=_perceptual(opt, device), ema_decay=p["ema_decay"], lr_gamma=p["lr_gamma"])
    if opt.captured:
        lips = 3 * len(ds.lips_shapes()) if opt.finetune_lips else (3 if opt.patch_size > 1 else 0)
        trainer = GraphedTrainer(model, opt, lips_graphs=lips, **kw)
    else:
        trainer = Trainer(model, opt, **kw)

    epoch0 = 0
    path = _which_checkpoint(opt, log)
    if path is not None:
        load_checkpoint(model, path, map_location=device, optimizer=trainer.optimizer, ema=trainer.ema)
        meta = getattr(model, "checkpoint_meta", {})
        epoch0, trainer.global_step = int(meta.get("epoch", 0)), int(meta.get("global_step", 0))
        if not trainer._device_schedule and trainer.lr_gamma is not None:      # the host route's rate of the next step under THIS run's iters
            for g in trainer.optimizer.param_groups:
                g["lr"] = g["initial_lr"] * trainer.lr_gamma ** (trainer.global_step / trainer.iters)
        log(f"[INFO] continuing from {path}: epoch {epoch0}, step {trainer.global_step}")
    cur = trainer.optimizer.current_lr() if hasattr(trainer.optimizer, "current_lr") else [g["lr"] for g in trainer.optimizer.param_groups]
    done.update(first_epoch=epoch0 + 1, start_step=trainer.global_step, start_lr=[float(v) for v in cur], trainer=trainer)

    val = _val_set(opt, device, "val", decode)
    model.mark_untrained_grid(ds.poses, ds.intrinsics)
    os.makedirs(os.path.join(opt.workspace, "checkpoints"), exist_ok=True)
    epoch = epoch0
    for epoch in range(epoch0 + 1, p["epochs"] + 1):
        losses = []
        for i in ds.order(epoch):
            if opt.finetune_lips:
                data = lips_schedule(ds, [i], trainer.global_step)
            elif opt.patch_size > 1:
                data = ds.batch_patch([i], opt.patch_size)
            else:
                data = ds.batch([i])
            losses.append(trainer.step(data))
        ds.check()                                                   # one word read back per epoch
        losses = torch.stack([l.reshape(()) for l in losses]).float().cpu().tolist()
        done["losses"].extend(losses)
        log(f"[INFO] epoch {epoch}: step {trainer.global_step}, mean loss {sum(losses) / len(losses):.6f}")
        ckpt = checkpoint_path(opt.workspace, epoch, opt.name)
        save_checkpoint(model, ckpt, ema=trainer.ema, optimizer=trainer.optimizer.state_dict(), epoch=epoch, global_step=trainer.global_step)
        done["checkpoints"].append(ckpt)
        if epoch % p["eval_interval"] == 0:
            done["evals"].append((epoch, _evaluate(trainer, val, log, f"val, epoch {epoch}")))
    done.update(epoch=epoch, global_step=trainer.global_step)

    # main.py:237-247: the test split with the averaged weights -- metrics when it carries its own frames, then the clip
    del ds
    torch.cuda.empty_cache()
    if opt.aud == "" and not opt.aud_wav:
        val.install(model)
        done["evals"].append((epoch, _evaluate(trainer, val, log, "test")))
    if opt.aud_wav:
        wav_features(opt, model, device, log)
    with trainer.eval_scope():
        done["video"], done["n_frames"] = render_clip(opt, model, device, results_dir, f"{opt.name}_ep{epoch:04d}", log, decode)
    done["avi"] = avi_path(results_dir, f"{opt.name}_ep{epoch:04d}") if opt.video and done["video"] else None
    return done


if __name__ == "__main__":
    main(sys.argv[1:])
