"""Stage 2 (VQA fine-tune) on MI355X: the Gemma3 step with the LLM, the projector and / or the vision tower trained.

Three of the reference's Stage-2 modes run here (QLoRA is not supported):
  A  --unfreeze_llm                                   (BASELINE cfg4; the default)   AdamW over the LLM
  B  --unfreeze_llm --unfreeze_projection_layer                                      AdamW over LLM + projector
  C  --unfreeze_projection_layer (LLM frozen)                                        AdamW over the projector
each with the vision tower frozen (the default) or trained as well (train_vision=True, which is also valid alone).
Mode A is described first; the trainable projector of B and C and the trainable tower follow below.

The body of `with self.accelerator.accumulate(...)` in VQATrainerStage2.train
(Stage2/trainer.py:299-444) with the cfg4 flags (`--unfreeze_llm`; projector
and vision encoder frozen; no QLoRA):

  SigLIP fwd (frozen, :313-332)          ptk_siglip_fwd
  projector fwd (frozen, :336-337)       ptk_projector_fwd -> the LLM input's vision rows
  [proj ‖ E[q]·s ‖ E[a]·s], mask, labels (:339-396)   inside ptk_gemma3_train_fwd_bwd
  Gemma3 fwd + manual CE (:398-418)      ptk_gemma3_train_fwd_bwd (label_offset = question length)
  accelerator.backward(loss / gas) (:421-423)   same call: dX and EVERY weight grad, accumulated into
                                         the bf16 .grad buffer (loss scaled 1/gas^2)
  sync: DDP grad reduce                  ZeRO-1: RCCL reduce-scatter of the flat bf16 grads
  clip_grad_norm_(llm, 1.0) + AdamW (:426-442)   ptk_bf16_grad_scale_sumsq + all-reduce of the sum of
                                         squares + ptk_adamw_bf16 on the rank's shard, then RCCL
                                         all-gather of the updated parameters
  lr_scheduler.step() x num_processes    host-side cosine-with-warmup lambda

Parameter stores: under `--mixed_precision bf16` the reference holds every trained module in bf16 (the LLM and
the tower loaded so, train_vqa_stage2.py:141-153,180-187; the projector cast, :274), so parameters, grads and
AdamW moments are bf16 tensors with no fp32 master, and the optimizer rounds every tensor op to bf16 as torch's
AdamW does on bf16 parameters.  Each trained module keeps exactly that in one `FlatStore` (flat_store.py) in the
kernel layouts, the module's tensors rebound onto views of it: `Gemma3TrainState` (q|k|v fused, gate/up
interleaved per 16 rows), `ProjectorTrainState` ([W1 | b1 | W2 | b2]) and `SiglipTrainState` (q|k|v rows fused,
the conv weight flattened).  The derived copies the kernels read (transposes for the dX GEMMs, the fp32 mirror of
norm weights / biases / positions) are refreshed after each optimizer step.

The optimizer step clips each trained module on its own norm (:437-439) and applies ptk_adamw_bf16 to each with
the shared LR / step count.  The LLM's store is ZeRO-1 sharded, its moments being the engine's shards.  The
projector's and the tower's are replicated and own their moments: at world > 1 their grads are summed by one
all-reduce (44 MB of bf16 for the projector's 22 M parameters, ~0.6 GB for the L/16 tower, next to the LLM's 2 GB
reduce-scatter; the tower's cost is unmeasured), scaled by 1 / world before the sum of squares, and every rank
takes the same deterministic step, so the replicas stay bit-identical without a parameter exchange.

Trainable projector (Stage2/trainer.py:214-223 collects its parameters, :336-337 runs it with grad; modes B, C).
Per micro-batch, after the Gemma3 call:
  dy = bf16(dx[vision rows]), patch 0's row zero          ptk_gather_vision_grad
  db2, dW2, dA = bf16((dy W2) gelu'(a)), db1, dW1         ptk_projector_bwd_bf16: each G rounded once to bf16 and
                                                          accumulated as autograd does, bf16(grad + bf16(G))
The forward is the frozen projector's (ptk_projector_fwd, bf16 GEMMs, output rounded to bf16), reading W1 / W2 from
the store.  Mode C builds no Gemma3TrainState: the LLM keeps the k-step-tiled frozen weights it was built with and
runs ptk_gemma3_loss_fwd_bwd (loss and dX only, label_offset = the question length).

Trainable vision tower (train_vision=True; the reference's --unfreeze_vision_encoder / first-epoch fine-tune,
Stage2/trainer.py:214-237,267-289, whose two flags exclude each other in its run script, so the tower never
trains there and no recorded step exists to match: the yardstick is torch autograd through
oracle.stage1_ref.siglip_vision_forward).  Per micro-batch:
  SigLIP fwd keeping activations                           ptk_siglip_train_fwd (bit-identical to ptk_siglip_fwd)
  ... projector fwd, Gemma3 fwd / loss / bwd as above ...
  dy = bf16(dx[vision rows]), patch 0's row zero           ptk_gather_vision_grad
  [db2, dW2,] dA, [db1, dW1,] d(vis) = bf16(dA W1)         ptk_projector_input_grad (one dA for both uses; the four
                                                           grads only when the projector is trained)
  every tower grad, accumulated bf16(grad + bf16(G))       ptk_siglip_bwd; d(vis) is d(last_hidden_state), its
                                                           patch-0 rows zero ([:, 1:] drops that patch)
With train_vision=False none of this runs and nothing the engine computes changes.
set_vision_trainable(False) freezes the tower again (frozen forward, no tower backward, no tower step) while
keeping its store, moments and the step count: the hook for a first-epoch-only schedule.
"""
from __future__ import annotations

import torch
import torch.distributed as dist

from . import _lib as L
from . import kernels as K
from .dist import all_gather_, all_reduce_bf16_sum_, reduce_scatter_
from .flat_store import FlatStore
from .gemma3 import Gemma3CausalLM
from .projectors import MLPProjector
from .siglip import SiglipVisionTower
from .stage1 import cosine_lambda

LAYER_KEYS = ("wqkv", "wo", "wgu", "wd", "ln_in", "ln_post_attn", "ln_pre_ff", "ln_post_ff", "q_norm", "k_norm")
LAYER_MATS = ("wqkv", "wo", "wgu", "wd")
NORM_KEYS = ("ln_in", "ln_post_attn", "ln_pre_ff", "ln_post_ff", "q_norm", "k_norm")
HF_NORM = {"ln_in": "input_layernorm", "ln_post_attn": "post_attention_layernorm",
           "ln_pre_ff": "pre_feedforward_layernorm", "ln_post_ff": "post_feedforward_layernorm",
           "q_norm": "self_attn.q_norm", "k_norm": "self_attn.k_norm"}
PROJ_KEYS = ("model.0.weight", "model.0.bias", "model.2.weight", "model.2.bias")   # Stage1/projectors.py's names


def deinterleave_gate_up(wgu):
    """[2I, H] interleaved per 16 rows -> gate [I, H], up [I, H] (inverse of gemma3.interleave_gate_up)."""
    I2, H = wgu.shape
    v = wgu.view(I2 // 32, 2, 16, H)
    return v[:, 0].reshape(I2 // 2, H), v[:, 1].reshape(I2 // 2, H)


class Gemma3TrainState(FlatStore):
    """Flat bf16 parameter / grad store of an unfrozen Gemma3CausalLM (rebinds the model's tensors).  The AdamW
    moments are ZeRO-1 shards and live in the engine."""

    def __init__(self, llm: Gemma3CausalLM, world_size: int = 1):
        self.llm, self.world = llm, world_size
        # matrices first, then every norm weight in the mirrored region (the norm kernels read them in fp32)
        segs = [("embed", llm.embed.shape)]
        for i, lay in enumerate(llm.layers):
            segs += [(f"{i}.{k}", lay[k].shape) for k in LAYER_MATS]
        norm_segs = [("final_norm", (llm.cfg.hidden_size,))]
        for i, lay in enumerate(llm.layers):
            norm_segs += [(f"{i}.{k}", lay[k].shape) for k in NORM_KEYS]
        super().__init__(segs, norm_segs, device=llm.device, pad_to=64 * world_size)   # equal ZeRO shards
        # copy the current weights in (bf16 matrices as they are; norm weights rounded to bf16, as the
        # reference's bf16-loaded model holds them), then rebind the model onto views of the store
        self.view("embed").copy_(llm.embed)
        self.view("final_norm").copy_(llm.final_norm)
        for i, lay in enumerate(llm.layers):
            for k in LAYER_KEYS:
                self.view(f"{i}.{k}").copy_(lay[k])
        llm.embed = self.view("embed")
        llm.final_norm = self.mirror_view("final_norm")
        for i, lay in enumerate(llm.layers):
            for k in LAYER_MATS:
                lay[k] = self.view(f"{i}.{k}")
            for k in NORM_KEYS:
                lay[k] = self.mirror_view(f"{i}.{k}")
        llm.drop_ktiled()
        self.refresh()
        llm._build_c()
        self._build_grads_c()

    def _build_grads_c(self):
        arr = (L.Gemma3LayerGradsC * len(self.llm.layers))()
        for i in range(len(self.llm.layers)):
            arr[i] = L.Gemma3LayerGradsC(*[self.grad_view(f"{i}.{k}").data_ptr() for k in LAYER_KEYS])
        self._c_layer_grads = arr
        self.c_grads = L.Gemma3GradsC(self.grad_view("embed").data_ptr(), self.grad_view("final_norm").data_ptr(),
                                      arr)

    def refresh(self):
        """Derived copies the kernels read: transposed matrices (dX GEMMs) and fp32 norm weights."""
        llm = self.llm
        self.refresh_mirror()
        for lay in llm.layers:
            for k in LAYER_MATS:
                K.transpose(lay[k], out=lay[k + "_t"])
        K.transpose(llm.embed, out=llm.embed_t)

    def shard(self, rank):
        n = self.numel // self.world
        return rank * n, n

    def state_dict_hf(self, grads=False):
        """HF Gemma3ForCausalLM names (lm_head tied, not listed), bf16 tensors on the device."""
        cfg = self.llm.cfg
        v = self.grad_view if grads else self.view
        Dq, Dkv = cfg.q_dim, cfg.kv_dim
        sd = {"model.embed_tokens.weight": v("embed")}
        for i in range(len(self.llm.layers)):
            p = f"model.layers.{i}."
            wqkv = v(f"{i}.wqkv")
            sd[p + "self_attn.q_proj.weight"] = wqkv[:Dq]
            sd[p + "self_attn.k_proj.weight"] = wqkv[Dq:Dq + Dkv]
            sd[p + "self_attn.v_proj.weight"] = wqkv[Dq + Dkv:]
            sd[p + "self_attn.o_proj.weight"] = v(f"{i}.wo")
            g, u = deinterleave_gate_up(v(f"{i}.wgu"))
            sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"] = g, u
            sd[p + "mlp.down_proj.weight"] = v(f"{i}.wd")
            for k in NORM_KEYS:
                sd[p + HF_NORM[k] + ".weight"] = v(f"{i}.{k}")
        sd["model.norm.weight"] = v("final_norm")
        return sd


class ProjectorTrainState(FlatStore):
    """Flat bf16 parameter / grad / moment store of a trainable Stage-2 projector: [W1 | b1 | W2 | b2], rounded
    from whatever the module holds.  The kernels read W1 and W2 from the store itself; W2^T (the dA GEMM's
    operand) and the fp32 biases ptk_projector_fwd takes are derived copies, refreshed after each optimizer step
    (the biases sit between the matrices, so they are copied one by one and not through a mirrored region).
    Stage 1's MLPProjector (fp32 masters, `flat` / `flat_grad`) is only read here, never changed."""

    def __init__(self, proj: MLPProjector, device):
        Dv, I, Dl = proj.vision_dim, proj.inter_dim, proj.llm_dim
        self.dims = (Dv, I, Dl)
        super().__init__(zip(PROJ_KEYS, ((I, Dv), (I,), (Dl, I), (Dl,))), device=device, moments=True)
        for name, p in zip(PROJ_KEYS, (proj.w1, proj.b1, proj.w2, proj.b2)):
            K.cast_bf16(p.detach().to(device=device, dtype=torch.float32).contiguous(), self.view(name))
        self.w2t = torch.empty((I, Dl), dtype=torch.bfloat16, device=device)
        self.bias32 = torch.zeros(I + Dl, dtype=torch.float32, device=device)
        self.tail = torch.zeros(L.lib().ptk_gemm_tail_scratch_bytes(), dtype=torch.uint8, device=device)
        self.c = L.ProjectorC(Dv, I, Dl, self.view(PROJ_KEYS[0]).data_ptr(), self.bias32.data_ptr(),
                              self.view(PROJ_KEYS[2]).data_ptr(), self.bias32[I:].data_ptr(), self.w2t.data_ptr(),
                              self.tail.data_ptr())
        self.refresh()

    def refresh(self):
        """Derived copies the kernels read: W2^T and the fp32 biases."""
        I = self.dims[1]
        K.transpose(self.view(PROJ_KEYS[2]), out=self.w2t)
        self.bias32[:I].copy_(self.view(PROJ_KEYS[1]))
        self.bias32[I:].copy_(self.view(PROJ_KEYS[3]))

    def state_dict(self, grads=False):
        """The reference's names (Stage1/projectors.py: model.0.weight, model.0.bias, model.2.weight,
        model.2.bias), bf16 tensors on the device (views of the store)."""
        return {k: self.view(k, self.grad if grads else None) for k in PROJ_KEYS}


SIGLIP_MATS = ("wqkv", "wo", "w1", "w2")
SIGLIP_TOP_SMALL = ("patch_b", "pos", "post_w", "post_b")
SIGLIP_SMALL = ("bqkv", "bo", "b1", "b2", "ln1_w", "ln1_b", "ln2_w", "ln2_b")
SIGLIP_GRAD_KEYS = ("wqkv", "bqkv", "wo", "bo", "w1", "b1", "w2", "b2", "ln1_w", "ln1_b", "ln2_w", "ln2_b")
SIGLIP_HF = {"wo": "self_attn.out_proj.weight", "bo": "self_attn.out_proj.bias", "w1": "mlp.fc1.weight",
             "b1": "mlp.fc1.bias", "w2": "mlp.fc2.weight", "b2": "mlp.fc2.bias", "ln1_w": "layer_norm1.weight",
             "ln1_b": "layer_norm1.bias", "ln2_w": "layer_norm2.weight", "ln2_b": "layer_norm2.bias"}


class SiglipTrainState(FlatStore):
    """Flat bf16 parameter / grad / moment store of a trained SigLIP tower (rebinds the tower's tensors): the
    matrices first (q|k|v rows fused, the conv weight flattened (c, ky, kx)), then the positions, biases and
    LayerNorm parameters in the mirrored region.  The tower's GEMM weights become views of the store; its fp32
    positions / biases / LN parameters, which the forward kernels read, become views of the fp32 mirror.  The
    k-step-tiled weight copies are dropped: they are copies of frozen weights.  ptk_siglip_bwd accumulates into
    the grad buffer."""

    def __init__(self, tower: SiglipVisionTower):
        self.tower = tower
        nl = len(tower.layers)
        segs = [("patch_w", tower.patch_w.shape)]
        for i, lay in enumerate(tower.layers):
            segs += [(f"{i}.{k}", lay[k].shape) for k in SIGLIP_MATS]
        small = [(k, getattr(tower, k).shape) for k in SIGLIP_TOP_SMALL]
        for i, lay in enumerate(tower.layers):
            small += [(f"{i}.{k}", lay[k].shape) for k in SIGLIP_SMALL]
        super().__init__(segs, small, device=tower.device, moments=True)
        # the current weights in (the fp32 ones rounded to bf16, as the reference's bf16-loaded tower holds them),
        # then the tower rebound onto views of the store / of the fp32 mirror
        for name, _ in segs + small:
            self.view(name).copy_(self._tower_tensor(name))
        tower.patch_w = self.view("patch_w")
        for k in SIGLIP_TOP_SMALL:
            setattr(tower, k, self.mirror_view(k))
        for i, lay in enumerate(tower.layers):
            for k in SIGLIP_MATS:
                lay[k] = self.view(f"{i}.{k}")
            for k in SIGLIP_SMALL:
                lay[k] = self.mirror_view(f"{i}.{k}")
        self.refresh()
        tower._build_c(ktiled=False)
        arr = (L.SiglipLayerGradsC * nl)()
        for i in range(nl):
            arr[i] = L.SiglipLayerGradsC(*[self.grad_view(f"{i}.{k}").data_ptr() for k in SIGLIP_GRAD_KEYS])
        self._c_layer_grads = arr
        self.c_grads = L.SiglipGradsC(*[self.grad_view(k).data_ptr() for k in ("patch_w",) + SIGLIP_TOP_SMALL], arr)
        self._ws = None

    def _tower_tensor(self, name):
        if "." in name:
            i, k = name.split(".")
            return self.tower.layers[int(i)][k]
        return getattr(self.tower, name)

    def refresh(self):
        """The fp32 copies the forward kernels read (positions, biases, LN parameters)."""
        self.refresh_mirror()

    def workspace(self, batch):
        """Saved activations + backward scratch of ptk_siglip_train_fwd / ptk_siglip_bwd at this batch."""
        n = L.lib().ptk_siglip_train_workspace_bytes(self.tower.c_cfg, batch)
        return L.grow(self, "_ws", n, self.tower.device)

    def state_dict_hf(self, grads=False):
        """HF SiglipVisionModel names (`vision_model.*`), bf16 tensors on the device: q|k|v split again, the conv
        weight as [D, C, P, P]."""
        c = self.tower.cfg
        v = self.grad_view if grads else self.view
        D, p = c.hidden_size, "vision_model."
        sd = {p + "embeddings.patch_embedding.weight": v("patch_w").view(D, c.num_channels, c.patch_size,
                                                                          c.patch_size),
              p + "embeddings.patch_embedding.bias": v("patch_b"),
              p + "embeddings.position_embedding.weight": v("pos"),
              p + "post_layernorm.weight": v("post_w"), p + "post_layernorm.bias": v("post_b")}
        for i in range(len(self.tower.layers)):
            q = f"{p}encoder.layers.{i}."
            wqkv, bqkv = v(f"{i}.wqkv"), v(f"{i}.bqkv")
            for j, n in enumerate("qkv"):
                sd[q + f"self_attn.{n}_proj.weight"] = wqkv[j * D:(j + 1) * D]
                sd[q + f"self_attn.{n}_proj.bias"] = bqkv[j * D:(j + 1) * D]
            for k, hf in SIGLIP_HF.items():
                sd[q + hf] = v(f"{i}.{k}")
        return sd


class Stage2Engine:
    """One VQATrainerStage2 micro-batch (forward_backward) and optimizer step (optimizer_step).

    train_llm / train_projector select the reference's Stage-2 modes; train_vision=True trains the SigLIP tower
    as well (with any of them, or alone):
      A  train_llm=True,  train_projector=False   ptk_gemma3_train_fwd_bwd; AdamW over the LLM (the default)
      B  train_llm=True,  train_projector=True    the same, then ptk_projector_bwd_bf16; AdamW over both
      C  train_llm=False, train_projector=True    ptk_gemma3_loss_fwd_bwd (dX only, the LLM as it was built --
                                                  frozen, with its k-step-tiled weights; no Gemma3TrainState),
                                                  then ptk_projector_bwd_bf16; AdamW over the projector"""

    def __init__(self, vision: SiglipVisionTower, llm: Gemma3CausalLM, projector: MLPProjector, *,
                 learning_rate=1e-4, weight_decay=0.01, gradient_accumulation_steps=1, max_grad_norm=1.0,
                 warmup_steps=0, total_steps=1, betas=(0.9, 0.999), eps=1e-8, world_size=1, rank=0,
                 process_group=None, pad_token_id=None, zero1=None, train_llm=True, train_projector=False,
                 train_vision=False):
        if not train_llm and not train_projector and not train_vision:
            raise ValueError("No trainable parameters found. Stage2Engine needs train_llm, train_projector or "
                             "train_vision")
        self.vision, self.llm, self.proj = vision, llm, projector
        self.train_llm, self.train_projector = bool(train_llm), bool(train_projector)
        self.train_vision = bool(train_vision)
        self.device = vision.device
        self.lr0, self.wd, self.gas, self.max_norm = learning_rate, weight_decay, gradient_accumulation_steps, max_grad_norm
        self.warmup, self.total, self.betas, self.eps = warmup_steps, total_steps, betas, eps
        self.world, self.rank, self.pg = world_size, rank, process_group
        self.pad_token_id = llm.cfg.pad_token_id if pad_token_id is None else pad_token_id
        # zero1: reduce-scatter / sharded AdamW / all-gather through the process group (default: world > 1;
        # True at world 1 runs the same collectives on a one-rank group, which tests the RCCL path on one GPU)
        self.zero1 = world_size > 1 if zero1 is None else bool(zero1)
        if world_size > 1 and not self.zero1:
            # the optimizer step exchanges grads only through the reduce-scatter / all-gather of ZeRO-1; without
            # it every rank would update from its own grads and the replicas would drift apart
            raise ValueError("Stage2Engine: zero1=False is not supported with world_size > 1")
        # a frozen LLM (mode C) keeps the weights it was built with: no flat store, no grads, no moments
        self.state = Gemma3TrainState(llm, world_size) if self.train_llm else None
        o, n = self.state.shard(rank) if self.train_llm else (0, 0)
        self.shard_lo, self.shard_n = o, n
        self.exp_avg = torch.zeros(n, dtype=torch.bfloat16, device=self.device)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.bfloat16, device=self.device)
        shards = self.zero1 and self.train_llm
        self._shard_grad = torch.empty(n, dtype=torch.bfloat16, device=self.device) if shards else None
        self._shard_param = torch.empty(n, dtype=torch.bfloat16, device=self.device) if shards else None
        # a trained projector (modes B, C): its own bf16 store, replicated on every rank (22 M parameters next to
        # the LLM's 1 B: its grads are all-reduced whole and every rank takes the same AdamW step)
        self.pstate = ProjectorTrainState(projector, self.device) if self.train_projector else None
        self.proj_grad_norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        # a trained vision tower: its own bf16 store, replicated like the projector's (one all-reduce of its grads,
        # the same deterministic step on every rank).  set_vision_trainable(False) freezes it again without
        # dropping the store, the moments or the step count (a first-epoch-only schedule)
        self.vstate = SiglipTrainState(vision) if self.train_vision else None
        self.vision_trainable = self.train_vision
        self.vision_grad_norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._partial = torch.empty(L.lib().ptk_bf16_sumsq_partial_floats(), dtype=torch.float32, device=self.device)
        self.sumsq = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.opt_step = 0
        self.sched_step = 0
        self.last_lr = learning_rate * cosine_lambda(0, warmup_steps, total_steps)
        self._shape = None

    def _buffers(self, B, T):
        if self._shape == (B, T):
            return
        vc, tc = self.vision.cfg, self.llm.cfg
        N, Dv, Dl, I = vc.num_patches, vc.hidden_size, tc.hidden_size, self.proj.inter_dim
        Sp = Gemma3CausalLM.seq_pad(N - 1 + T)
        dev, bf = self.device, torch.bfloat16
        self.N, self.Sp = N, Sp
        self.px = torch.empty((B, vc.num_channels, vc.image_size, vc.image_size), dtype=bf, device=dev)
        self.vis = torch.empty((B * N, Dv), dtype=bf, device=dev)
        self.a = torch.empty((B * N, I), dtype=bf, device=dev)
        self.h = torch.empty((B * N, I), dtype=bf, device=dev)
        self.x = torch.empty((B * Sp, Dl), dtype=torch.float32, device=dev)
        self.dx = torch.empty((B * Sp, Dl), dtype=torch.float32, device=dev)
        self.vision.workspace(B)
        if self.vstate is not None:
            self.dvis = torch.empty((B * N, Dv), dtype=bf, device=dev)
            self.vstate.workspace(B)
        if self.pstate is not None or self.vstate is not None:
            self.dy = torch.empty((B * N, Dl), dtype=bf, device=dev)
            lib = L.lib()
            ws_fn = lib.ptk_projector_bwd_bf16_workspace_bytes if self.vstate is None else \
                lib.ptk_projector_input_grad_workspace_bytes
            L.grow(self, "_proj_ws", ws_fn(self._proj_c(), B * N), dev)
        ws_bytes = L.lib().ptk_gemma3_train_workspace_bytes if self.train_llm else L.lib().ptk_gemma3_workspace_bytes
        L.grow(self, "_ws", ws_bytes(self.llm.c_cfg, B, T, Sp), dev)
        self._shape = (B, T)

    def _proj_c(self):
        """The projector the kernels read: the trained store's, or the frozen module's bf16 shadows."""
        return self.pstate.c if self.pstate is not None else self.proj.desc()

    def set_vision_trainable(self, on):
        """Freeze (False) or unfreeze (True) a tower built with train_vision=True.  Frozen, later micro-batches
        take the frozen forward (no activations kept, no tower backward) and optimizer_step skips the tower; its
        store, moments and the shared step count are kept.  The hook for the reference's first-epoch-only
        vision-encoder fine-tune (Stage2/trainer.py:267-289)."""
        if on and self.vstate is None:
            raise ValueError("Stage2Engine: set_vision_trainable(True) needs an engine built with train_vision=True")
        self.vision_trainable = bool(on)

    def _inputs(self, pixel_values, question_ids, answer_ids, train=True):
        """Vision + projector rows of x, token ids and labels, and the batch descriptor."""
        B, Tq = question_ids.shape
        Ta = answer_ids.shape[1]
        T = Tq + Ta
        self._buffers(B, T)
        if tuple(pixel_values.shape) != tuple(self.px.shape):
            raise ValueError(f"pixel_values {tuple(pixel_values.shape)} do not match the vision tower's input "
                             f"{tuple(self.px.shape)}")
        if pixel_values.dtype == torch.bfloat16:
            self.px.copy_(pixel_values)
        else:
            K.cast_bf16(pixel_values.contiguous(), self.px)
        if train and self.vision_trainable:   # the same forward, keeping what the tower's backward reads
            self.vision.forward_train_into(self.px, self.vis, self.vstate)
        else:
            self.vision.forward_into(self.px, self.vis)
        if self.pstate is None:
            self.proj.fwd_into(self.vis, self.a, self.h, self.x, out_map=(self.N, 1, self.Sp, -1), round_bf16=True)
        else:   # the same forward from the engine's bf16 store (the parameters the optimizer updates)
            L.check(L.lib().ptk_projector_fwd(self.pstate.c, self.vis.shape[0], self.vis.data_ptr(),
                                              self.a.data_ptr(), self.h.data_ptr(), self.x.data_ptr(),
                                              L.RowMap(self.N, 1, self.Sp, -1), self.x.shape[1], 1,
                                              L.stream_ptr(self.device)), "ptk_projector_fwd")
        ids = torch.cat([question_ids, answer_ids], dim=1).contiguous()
        labels = answer_ids.masked_fill(answer_ids == self.pad_token_id, -100).contiguous()
        cfg = self.llm.c_cfg
        if self.pad_token_id != cfg.pad_token_id:
            cfg = L.Gemma3ConfigC.from_buffer_copy(cfg)
            cfg.pad_token_id = int(self.pad_token_id)
        bt = L.Gemma3BatchC(B, T, self.N - 1, self.Sp, ids.data_ptr(), labels.data_ptr(), self.x.data_ptr(),
                            self.dx.data_ptr(), 1.0 / float(self.gas * self.gas), self.loss.data_ptr(), Tq)
        self._ids, self._labels = ids, labels     # alive until the stream has consumed them
        return cfg, bt

    def forward_backward(self, pixel_values, question_ids, answer_ids):
        """One micro-batch: loss (device [1], the mean CE over answer tokens) and grads accumulated
        (scaled 1/gas^2: the trainer's loss / gas and Accelerator.backward's / gas)."""
        cfg, bt = self._inputs(pixel_values, question_ids, answer_ids)
        stream = L.stream_ptr(self.device)
        if self.train_llm:
            L.check(L.lib().ptk_gemma3_train_fwd_bwd(cfg, self.llm.c_w, bt, self.state.c_grads, self._ws.data_ptr(),
                                                     self._ws.numel(), stream), "ptk_gemma3_train_fwd_bwd")
        else:   # frozen LLM: loss and dX only
            L.check(L.lib().ptk_gemma3_loss_fwd_bwd(cfg, self.llm.c_w, bt, self._ws.data_ptr(), self._ws.numel(),
                                                    stream), "ptk_gemma3_loss_fwd_bwd")
        ps, B = self.pstate, question_ids.shape[0]
        if ps is not None or self.vision_trainable:
            # dy = bf16(dx[vision rows]) (patch 0's row zero)
            L.check(L.lib().ptk_gather_vision_grad(self.dx.data_ptr(), B, self.N, self.Sp, self.x.shape[1],
                                                   self.dy.data_ptr(), stream), "gather_vision_grad")
        g = [t.data_ptr() for t in ps.state_dict(grads=True).values()] if ps is not None else [None] * 4
        if self.vision_trainable:
            # the projector's four grads (when it is trained) and its input grad d(vis) from one dA, then the
            # tower's backward: d(last_hidden_state), whose patch-0 rows are zero (dy's are)
            L.check(L.lib().ptk_projector_input_grad(self._proj_c(), B * self.N, self.vis.data_ptr(),
                                                     self.a.data_ptr(), self.h.data_ptr(), self.dy.data_ptr(), *g,
                                                     self.dvis.data_ptr(), self._proj_ws.data_ptr(),
                                                     self._proj_ws.numel(), stream), "ptk_projector_input_grad")
            self.vision.backward(self.dvis, self.vstate)
        elif ps is not None:
            # the four grads accumulated into the bf16 .grad
            L.check(L.lib().ptk_projector_bwd_bf16(ps.c, B * self.N, self.vis.data_ptr(), self.a.data_ptr(),
                                                   self.h.data_ptr(), self.dy.data_ptr(), *g,
                                                   self._proj_ws.data_ptr(), self._proj_ws.numel(), stream),
                    "ptk_projector_bwd_bf16")
        return self.loss

    def forward_loss(self, pixel_values, question_ids, answer_ids):
        """Validation loss under no_grad (Stage2/trainer.py:518-591): forward + CE only, no grads touched."""
        cfg, bt = self._inputs(pixel_values, question_ids, answer_ids, train=False)
        L.check(L.lib().ptk_gemma3_loss_fwd(cfg, self.llm.c_w, bt, self._ws.data_ptr(), self._ws.numel(),
                                            L.stream_ptr(self.device)), "ptk_gemma3_loss_fwd")
        return self.loss

    def optimizer_step(self):
        """DDP grad average (ZeRO-1 reduce-scatter), clip_grad_norm_(max_norm), AdamW, all-gather, schedule.
        The LLM (when trained) and the projector (when trained) are clipped each on its own norm
        (Stage2/trainer.py:437-439) and share the LR, betas, eps, weight decay and step count."""
        lr = self.lr0 * cosine_lambda(self.sched_step, self.warmup, self.total)
        self.opt_step += 1
        if self.train_llm:
            self._llm_step(lr)
        if self.pstate is not None:
            self._replicated_step(self.pstate, self.proj_grad_norm, lr)
        if self.vision_trainable:
            self._replicated_step(self.vstate, self.vision_grad_norm, lr)
        self.sched_step += self.world
        self.last_lr = lr       # the LR this optimizer step used (param_groups[0]["lr"] during .step())
        return lr

    def _clip_adamw(self, p, g, exp_avg, exp_avg_sq, n, scale, sumsq, norm_out, lr, sum_over_ranks=False):
        """g *= scale and its sum of squares into `sumsq` (summed over the ranks' shards when asked), then the
        clip on that norm (written to `norm_out`) and bf16 AdamW on p, with the engine's shared betas, eps, weight
        decay, max norm and step count."""
        stream = L.stream_ptr(self.device)
        L.check(L.lib().ptk_bf16_grad_scale_sumsq(g.data_ptr(), n, scale, self._partial.data_ptr(),
                                                  sumsq.data_ptr(), stream), "grad_scale_sumsq")
        if sum_over_ranks:
            dist.all_reduce(sumsq, op=dist.ReduceOp.SUM, group=self.pg)
        b1, b2 = self.betas
        L.check(L.lib().ptk_adamw_bf16(p.data_ptr(), g.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), n,
                                       sumsq.data_ptr(), self.max_norm, lr, b1, b2, self.eps, self.wd,
                                       self.opt_step, norm_out.data_ptr(), stream), "adamw_bf16")

    def _llm_step(self, lr):
        """ZeRO-1: reduce-scatter of the grads, clip + AdamW on this rank's shard, all-gather of the parameters."""
        st = self.state
        lo, n = self.shard_lo, self.shard_n
        if self.zero1:
            reduce_scatter_(self._shard_grad, st.grad, self.world, self.rank, self.pg)
            g, scale = self._shard_grad, 1.0 / self.world
        else:
            g, scale = st.grad, 1.0
        p = st.flat[lo:lo + n]
        self._clip_adamw(p, g, self.exp_avg, self.exp_avg_sq, n, scale, self.sumsq, self.grad_norm, lr,
                         sum_over_ranks=self.zero1)
        if self.zero1:
            self._shard_param.copy_(p)
            all_gather_(st.flat, self._shard_param, self.world, self.pg)
        st.refresh()
        st.zero_grad()

    def _replicated_step(self, store, norm_out, lr):
        """A replicated module's own clip + AdamW on its whole store (the projector, the tower;
        Stage2/trainer.py:433-439 clips each trained module separately): at world > 1 the ranks' grads are summed
        by one all-reduce (every rank receives the same bits), scaled by 1 / world before the sum of squares as
        the LLM's shards are, and every rank takes the same deterministic step, so the replicas stay
        bit-identical without a parameter exchange."""
        scale = 1.0
        if self.zero1:
            all_reduce_bf16_sum_(store.grad, self.pg)
            scale = 1.0 / self.world
        self._clip_adamw(store.flat, store.grad, store.exp_avg, store.exp_avg_sq, store.numel, scale, store.sumsq,
                         norm_out, lr)
        store.refresh()
        store.zero_grad()

    @property
    def scheduler_lr(self):
        """lr_scheduler.get_last_lr()[0]: the LR after the scheduler stepped num_processes times per optimizer
        step, i.e. the next step's LR -- what the reference logs as train/learning_rate
        (Stage2/trainer.py:446-452)."""
        return self.lr0 * cosine_lambda(self.sched_step, self.warmup, self.total)

    # ------------------------------------------------------------------ optimizer state (ZeRO-1 shards)
    def optimizer_state(self):
        """This rank's optimizer shard (moments of params [shard_lo, shard_lo + shard_n) of the flat store)
        plus the step / schedule counters: every rank's file together is the full AdamW state."""
        sd = {"exp_avg": self.exp_avg.cpu(), "exp_avg_sq": self.exp_avg_sq.cpu(), "step": self.opt_step,
              "sched_step": self.sched_step, "shard": (self.shard_lo, self.shard_n), "world": self.world,
              "rank": self.rank, "numel": self._llm_numel}
        for key, st in self._replicated():   # their moments, whole on every rank (the stores are replicated)
            sd.update({f"{key}_exp_avg": st.exp_avg.cpu(), f"{key}_exp_avg_sq": st.exp_avg_sq.cpu(),
                       f"{key}_numel": st.numel})
        return sd

    @property
    def _llm_numel(self):
        return self.state.numel if self.train_llm else 0

    def _replicated(self):
        """(checkpoint key prefix, store) of the replicated stores this engine was built with."""
        return [(key, st) for key, st in (("proj", self.pstate), ("vision", self.vstate)) if st is not None]

    def load_optimizer_state(self, sd):
        pn, vn = (0 if st is None else st.numel for st in (self.pstate, self.vstate))
        if (sd["world"], sd["rank"], sd["numel"], sd.get("proj_numel", 0), sd.get("vision_numel", 0)) != (
                self.world, self.rank, self._llm_numel, pn, vn):
            raise ValueError(f"optimizer shard of world {sd['world']} rank {sd['rank']} (store {sd['numel']}, "
                             f"projector {sd.get('proj_numel', 0)}, vision {sd.get('vision_numel', 0)}) does not "
                             f"match this engine (world {self.world} rank {self.rank} store {self._llm_numel}, "
                             f"projector {pn}, vision {vn})")
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        for key, st in self._replicated():
            st.exp_avg.copy_(sd[f"{key}_exp_avg"])
            st.exp_avg_sq.copy_(sd[f"{key}_exp_avg_sq"])
        self.opt_step, self.sched_step = int(sd["step"]), int(sd["sched_step"])

    def projector_state_dict(self, grads=False):
        """The trained projector's parameters (or accumulated grads) under the reference's names, bf16 on the
        device -- what Gemma3TrainState.state_dict_hf is for the LLM."""
        if self.pstate is None:
            raise ValueError("Stage2Engine: the projector is frozen (train_projector=False)")
        return self.pstate.state_dict(grads)


    def vision_state_dict(self, grads=False):
        """The trained tower's parameters (or accumulated grads) under HF's names, bf16 on the device."""
        if self.vstate is None:
            raise ValueError("Stage2Engine: the vision tower is frozen (train_vision=False)")
        return self.vstate.state_dict_hf(grads)


def synthetic_engine(cfg, device="cuda", seed=0, **kw):
    """Stage2Engine over random-init towers of the named architecture (benchmark; no checkpoints offline)."""
    vision = SiglipVisionTower.random_init(cfg.vision, device, seed)
    llm = Gemma3CausalLM.random_init(cfg.text, device, seed + 1, max_pos=Gemma3CausalLM.seq_pad(cfg.seq_len),
                                     frozen=not kw.get("train_llm", True))   # trained: no k-step-tiled copies
    torch.manual_seed(seed + 2)
    proj = MLPProjector(cfg.vision.hidden_size, cfg.text.hidden_size, cfg.expansion_factor, device=device)
    return Stage2Engine(vision, llm, proj, **kw)
