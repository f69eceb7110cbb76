"""Worker body of the world-2 tests of Stage 2 with a trainable projector (spawned by tests/test_stage2_proj_gpu.py)."""
import os

import numpy as np
import torch
import torch.distributed as dist

from tests.dist_worker import _init


def stage2_proj(rank, world, port, out_dir, train_llm):
    """GPU (one device shared) / gloo: Stage2Engine with train_projector=True (and the LLM trained or frozen); each
    rank runs its 2 samples of a batch of 2 * world, then the optimizer step.  Saves the replica's projector store,
    its norm and, when the LLM is trained, the LLM's flat parameters and norm."""
    _init(rank, world, port, "gloo")
    from projectiontrainer_amd import weights as W
    from projectiontrainer_amd.config import PRESETS
    from projectiontrainer_amd.stage2 import synthetic_engine
    dev = torch.device("cuda:0")
    cfg = PRESETS["tiny"].replace(batch_size=2 * world, text_len=8 + 12, question_len=8)
    torch.manual_seed(0)
    eng = synthetic_engine(cfg, dev, seed=3, world_size=world, rank=rank, learning_rate=1e-3, total_steps=10,
                           train_llm=train_llm, train_projector=True)
    px, q, a = (torch.from_numpy(t).to(dev) for t in W.synthetic_vqa_batch(cfg, seed=9))
    sl = slice(2 * rank, 2 * rank + 2)
    eng.forward_backward(px[sl], q[sl], a[sl])
    eng.optimizer_step()
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, f"proj{rank}.npy"), eng.pstate.flat.float().cpu().numpy())
    np.save(os.path.join(out_dir, f"projnorm{rank}.npy"), eng.proj_grad_norm.cpu().numpy())
    if train_llm:
        np.save(os.path.join(out_dir, f"llm{rank}.npy"), eng.state.flat.float().cpu().numpy())
        np.save(os.path.join(out_dir, f"llmnorm{rank}.npy"), eng.grad_norm.cpu().numpy())
    dist.destroy_process_group()
