"""The stability rule and batch picker of the fp32 head tests (tests/headref32.py) on the CPU, with the model alone: the
batches tests/test_gpu_train_head_ref.py compares gradients on exist, their rows pass the rule, and the rule excludes the
share of uniformly drawn samples that DESIGN section 4 records."""
import pytest
import torch

import headref32
import netref16
from netref64 import Net64Libm

_SCENES = {}
SEED0 = 3200                      # the seed of a batch of netref16.CASES[i] is SEED0 + i (tests/test_gpu_train_head_ref.py)


def _ref(tag):
    if tag not in _SCENES:
        _SCENES[tag] = Net64Libm(netref16.head_scene(tag, "cpu").model)
    return _SCENES[tag]


@pytest.mark.parametrize("case", range(len(netref16.CASES)))
def test_small_batches_exist_and_their_rows_pass_the_rule(case):
    """The pool's excluded share lies in 45 - 60 % (measured on 4096 uniform samples: 51.3 - 53.7 %; a pool of 4 M + 256 = 260
    .. 636 candidates scatters around that by 2 - 3 points), the pick succeeds (stable_batch32 asserts it), and the picked
    rows pass the rule evaluated on the batch itself -- all but the rows put outside the bound, which are kept whatever it says."""
    tag, M, live, _ = netref16.CASES[case]
    ref = _ref(tag)
    m = ref.model
    b = headref32.stable_batch32(ref, M, SEED0 + case)
    n, n_oob = (live if live is not None else M), min(2, M // 8)
    print(f"{tag} M={M} live={live}: pool excluded {b['pool_excluded']:.1%} " + " ".join(f"{k} {v:.1%}" for k, v in b["shares"].items()))
    assert b["xyzs"].shape == (M, 3) and b["dirs"].shape == (M, 3) and b["excluded"].shape == (M,)
    assert 0.45 <= b["pool_excluded"] <= 0.60
    again = headref32.unstable32(ref, b["xyzs"], b["dirs"], b["enc_a"], ref.P["individual_codes"][0].detach() if m.individual_dim else None,
                                 b["eye"] if m.exp_eye else None)["any"]
    assert torch.equal(again, b["excluded"])
    inside = torch.ones(M, dtype=torch.bool)
    inside[1:1 + n_oob] = False
    assert not bool(b["excluded"][inside].any())
    assert bool((b["xyzs"][~inside] == 1.25).all()) and bool((b["xyzs"][inside].abs() <= 0.98).all())
    assert 3 * int(b["excluded"][:n].sum()) <= n
    for u in b["up"]:                                    # excluded rows carry no upstream gradient, the others do
        assert float(u[b["excluded"]].abs().sum()) == 0.0 and bool((u[~b["excluded"]].reshape(M - int(b["excluded"].sum()), -1).abs().sum(-1) > 0).all())


@pytest.mark.parametrize("tag", ["default", "hash19", "noeye_noind"])
def test_share_of_uniform_samples_each_rule_excludes(tag):
    """4096 uniform samples (the pool of M = 960): the first three clauses 51.3 - 53.7 %, ReLU 2.9 - 4.3 %, ambient cells 44 - 47 %,
    xyz cells 9.1 - 9.5 % over three seeds of three models, asserted with one point of slack on either side; the clause behind
    the ambient grid is printed, and the whole rule stays within 45 - 60 %."""
    ref = _ref(tag)
    shares = headref32.stable_batch32(ref, 960, 77)["shares"]
    print(tag, " ".join(f"{k} {v:.1%}" for k, v in shares.items()))
    assert 0.45 <= shares["any"] <= 0.60
    assert 0.019 <= shares["relu"] <= 0.053 and 0.43 <= shares["ambient"] <= 0.48 and 0.081 <= shares["xyz"] <= 0.105
