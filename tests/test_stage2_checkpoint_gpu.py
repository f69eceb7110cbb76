"""The format of Stage2Engine.optimizer_state() (what optimizer_rank*.pt holds) with all three modules trained:
the exact key set, the shard and numel entries, a bit-exact load into a second engine, and the mismatch error.
Tiny towers with the 64-patch vision side of tests/test_stage2_vision_gpu.py: the tower's backward takes whole
64-row blocks, so config.py's tiny preset (16 patches) cannot train it."""
import pytest
import torch

from tests.test_optim_gpu import bits
from tests.test_stage2_vision_gpu import batch, engine

pytestmark = pytest.mark.gpu

KEYS = {"exp_avg", "exp_avg_sq", "step", "sched_step", "shard", "world", "rank", "numel",
        "proj_exp_avg", "proj_exp_avg_sq", "proj_numel", "vision_exp_avg", "vision_exp_avg_sq", "vision_numel"}


def test_optimizer_state_format_is_stable(gpu):
    e1 = engine(gpu, "llm_proj", True)
    e1.forward_backward(*batch(gpu))
    e1.optimizer_step()
    sd = e1.optimizer_state()
    assert set(sd) == KEYS
    assert sd["shard"] == (0, e1.state.numel)
    assert (sd["numel"], sd["proj_numel"], sd["vision_numel"]) == (e1.state.numel, e1.pstate.numel, e1.vstate.numel)
    assert (sd["step"], sd["sched_step"], sd["world"], sd["rank"]) == (1, 1, 1, 0)
    for key, n in (("", sd["numel"]), ("proj_", sd["proj_numel"]), ("vision_", sd["vision_numel"])):
        for m in (sd[key + "exp_avg"], sd[key + "exp_avg_sq"]):
            assert m.device.type == "cpu" and m.dtype == torch.bfloat16 and m.shape == (n,) and m.any()
    e2 = engine(gpu, "llm_proj", True)
    assert not e2.exp_avg.any() and e2.opt_step == 0
    e2.load_optimizer_state(sd)
    for got, want in ((e2.exp_avg, e1.exp_avg), (e2.exp_avg_sq, e1.exp_avg_sq),
                      (e2.pstate.exp_avg, e1.pstate.exp_avg), (e2.pstate.exp_avg_sq, e1.pstate.exp_avg_sq),
                      (e2.vstate.exp_avg, e1.vstate.exp_avg), (e2.vstate.exp_avg_sq, e1.vstate.exp_avg_sq)):
        assert torch.equal(bits(got), bits(want))
    assert (e2.opt_step, e2.sched_step) == (e1.opt_step, e1.sched_step) == (1, 1)
    bad = dict(sd, proj_numel=sd["proj_numel"] + 64)
    with pytest.raises(ValueError, match="does not match this engine"):
        e2.load_optimizer_state(bad)
