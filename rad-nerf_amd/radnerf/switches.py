"""The RN_* environment switches of the Python side, in one table; `get` / `on` are their only readers.

A switch is read when it is asked for (nothing is cached: tests and tools flip them between calls), a value outside its accepted
ones is a ValueError, and `python -m radnerf.switches` prints the table as the "Switches" section of INTEGRATION.md.  The tuning
knobs the C library reads for itself (csrc/) are not listed here."""
import os

# (name, default, accepted values, what the switch selects)
TABLE = (
    ("RN_ADAM", "hip", ("hip", "torch"), "optimizer of `make_optimizer` on the GPU: `HipAdam` (one update kernel for all tensors) or torch's fused Adam"),
    ("RN_ASR", "torch", ("torch", "hip"), "`Wav2Vec2CTC` (`radnerf/asr.py`) on the GPU in fp32: the same arithmetic in plain torch, or the wav2vec2 kernels (`rn_asr_*`, opt-in: bit-reproducible and independent of the batching, but 47.5 ms against 43.4 ms for a minute of audio at the real size and 11.4 ms against 6.5 ms for one live window, DESIGN.md §3)"),
    ("RN_ASR_TILE", "auto", ("auto", "32", "128"), "with `RN_ASR=hip`: tiling of the wav2vec2 matrix products: `128` (128 x 128 tiles through LDS), `32` (one wave per 32 x 32 tile, for the few rows of one live window) or per product from its shape and the device's compute-unit count; both tilings run the same chain over k per output, so the logits have the same bits under every value"),
    ("RN_AUDIO_TRAIN", "hip", ("hip", "torch"), "`encode_audio` on the GPU: the audio kernels (`radnerf/audio.py`) or the `nn.Module` path"),
    ("RN_DENSE_BUDGET_MB", "384", ("160", "384", "896", "2304"), "with `RN_DENSE_LEVELS=1`: the most memory, in MiB, the dense image of the xyz table may take (`opt.dense_budget_mb`, any number, overrides it); for the T = 2^19 hash grid in fp32 the four values store levels 5-8 (149 MiB), 5-9 (343 MiB), 5-10 (857 MiB) and 5-11 (2215 MiB) as lattices, fp16 tables take half"),
    ("RN_DENSE_LEVELS", "1", ("1", "0"), "fused inference engine: a frame whose xyz table is that of the frame before reads the coarser hashed levels from a dense image built once (`rn_grid_dense_build`: each such level stored as its whole lattice, so neighbouring samples share cache lines; same features, same bits); `0`: every frame gathers from the hashed table"),
    ("RN_DIR_TERM", "1", ("1", "0"), "fused inference engine, fp32 network kernel: the colour net's direction term (bias + 8 MFMA steps over SH(dir), the same for every sample of a ray) is stored per ray by the loop's first iteration and loaded by the later ones (`rn_head_t.dir_term`, 256 bytes per ray, frames of up to 2^20 rays; same bits); `0`: every sample computes it"),
    ("RN_LIVE_LIST", "1", ("1", "0"), "fused inference engine: hand the loop the list of live sample slots (`0`: every launch scans all slots)"),
    ("RN_MLP_TRAIN", "hip", ("hip", "torch"), "the per-operator MLP stacks under autograd: `rn_mlp64_*` (`radnerf/mlp_train.py`) or `nn.Linear`"),
    ("RN_OCC_BOX", "1", ("1", "0"), "fused inference engine: hand the loop the box around the occupancy grid's set bits (`rn_occ_box`, built once per grid): with one cascade and a constant step a ray tests only the cells between its entry into and its exit from that box (same bits); `0`: every ray tests every cell from `near` to `far`"),
    ("RN_PERCEP", "hip", ("hip", "torch"), "`PerceptualAlex` (`radnerf/percep.py`) on the GPU in fp32: the perceptual kernels (`rn_percep_*`), or the same arithmetic in plain torch (unfold + matmul)"),
    ("RN_SCATTER", "lbc", ("lbc", "binned"), "table-gradient scatter: the line merge for every level, or hashed levels of the first grid summed by table region"),
    ("RN_TORSO_PLAN", "1", ("1", "0"), "fused inference engine: a frame whose pixel grid and torso occupancy grid are those of the frame before runs its torso pass over a plan built once (`rn_torso_plan_build`: the covered pixels and their position encoding; same bits); `0`: every frame computes them (`rn_torso_blend_frame`)"),
    ("RN_TORSO_STEP", "device", ("device", "host"), "with `RN_TORSO_TRAIN=fused`: the whole torso step on a device-side count, or the fused layer on the index list the host asks for"),
    ("RN_TORSO_TRAIN", "ops", ("ops", "fused"), "torso layer of a training call: the per-operator layers, or the fused kernels of `radnerf/train_torso.py` (opt-in)"),
    ("RN_TRAIN_CAMERA", "torch", ("torch", "fused"), "pose code of `--train_camera`: torch's expressions, or `rn_camera_rays_*` (`radnerf/train_camera.py`, opt-in; lets a captured camera step keep the fused head)"),
    ("RN_TRAIN_DETERMINISTIC", "0", ("0", "1"), "`1`: a step on the fused routes (head, `RN_TRAIN_CAMERA=fused`, `RN_TORSO_TRAIN=fused`) runs no float atomic, eager or captured: the table gradients are summed in one fixed order (`rn_grid_scatter_ordered`; takes precedence over `RN_SCATTER`) and the audio nets' parameter gradients through per-workgroup partials -- two runs from the same seeds give the same bits (opt-in: slower)"),
    ("RN_TRAIN_GLUE", "hip", ("hip", "torch"), "elementwise glue of the per-operator step: single kernels (`radnerf/train_glue.py`) or the PyTorch expressions"),
    ("RN_TRAIN_HEAD", "fused", ("fused", "ops"), "`NeRFNetwork.forward` of a training call: one forward and one backward kernel (`radnerf/train_head.py`) or the per-operator path"),
    ("RN_TRAIN_HEAD_ZERO", "0", ("0", "1"), "`1`: the fused head zero-fills its output rows past the live count (for tools that look at all rows)"),
    ("RN_TRAIN_LOSS", "fused", ("fused", "torch"), "head loss of `train_step`: blend, clamp and loss in one kernel, or the PyTorch expression"),
    ("RN_TRAIN_MARCH", "step", ("step", "ops"), "marcher of a budgeted step: one launch with near / far and the counters, or `near_far_from_aabb` + `rn_march_rays_train_budget`"),
    ("RN_TRAIN_MLP", "f32", ("f32", "f16"), "matrix products of the fused head (`RN_TRAIN_HEAD=fused`): fp32 matrix cores, or 16-bit operands with fp32 sums (`rn_train_head_*_h16`, opt-in: the arithmetic of the reference's `-O` runs for its `nn.Linear` layers; saved tiles, tables and gradients stay fp32)"),
    ("RN_TRAIN_NOISE", "hash", ("hash", "torch"), "jitter of the one-launch marcher: the launch's own hash, or `torch.rand` as the reference draws it (the test suite pins this)"),
    ("RN_TRAIN_OVERLAP", "1", ("1", "0"), "table-gradient scatter and audio nets on side streams beside the step (`0`: everything on one stream)"),
    ("RN_TRAIN_PACKED", "1", ("1", "0"), "`SyntheticTrainStream.batch`: one gather kernel into one flat buffer (`0`: separate tensors, as a generic loader hands over)"),
    ("RN_TRAIN_SET", "hip", ("hip", "torch"), "`DeviceTrainSet.batch` on the GPU: one launch, or the plain-torch restatement of `collate`"),
)
_ROWS = {row[0]: row for row in TABLE}


def get(name):
    """The switch's value in the environment now, or its default; ValueError for a value it does not accept."""
    _, default, accepted, _ = _ROWS[name]
    value = os.environ.get(name, default)
    if value not in accepted:
        raise ValueError(f"{name}={value!r} is not one of its accepted values: {' | '.join(accepted)}")
    return value


def on(name):
    """get() of a `0 | 1` switch as a bool."""
    return get(name) == "1"


def markdown():
    rows = ["| switch | default | accepted | selects |", "|---|---|---|---|"]
    rows += ["| `%s` | `%s` | %s | %s |" % (name, default, " \\| ".join("`%s`" % v for v in accepted), doc) for name, default, accepted, doc in TABLE]
    return "\n".join(rows)


if __name__ == "__main__":
    print(markdown())
