"""The reference's two inference calls on already-constructed towers.

* `describe_images`: Stage1/inference_stage1.py:150-193 -- the projected image patches alone are the prompt
  (`generate(inputs_embeds=projected, attention_mask=ones, max_new_tokens=256, do_sample=True, temperature=0.7,
  top_p=0.9, repetition_penalty=1.0, pad_token_id=, eos_token_id=)`), the new tokens decoded with
  skip_special_tokens.
* `answer_question`: `process_sample`, Stage2/inference_vqa_stage2.py:211-281 -- the question tokenised with
  add_special_tokens=False, prompt = [projected patches | question embeddings], attention mask all ones,
  `generate(..., max_new_tokens=512, do_sample=True, temperature=0.3, top_p=0.9, top_k=50, repetition_penalty=1.8,
  length_penalty=1.2, num_beams=3)`, the first sequence decoded with skip_special_tokens.

The towers are the package's own: `SiglipVisionTower.__call__` (last_hidden_state, whose first token the scripts
drop), `MLPProjector.forward`, `Gemma3CausalLM.get_input_embeddings` / `generate` / `beam_generate`, and
`ImagePreprocessor` for the pixels (the script's `image.resize((s, s))` followed by the processor is one bicubic
resize to s x s, which is what ImagePreprocessor does).  The scripts run the projector and the LLM in bf16, so the
prompt rows are rounded to bf16 values (held in fp32, as the decode takes them); the projector itself runs in the
package's own precision (see project_images).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib as L
from .gemma3 import QLORA_UNSUPPORTED

STAGE1_DEFAULTS = dict(max_new_tokens=256, do_sample=True, temperature=0.7, top_p=0.9, repetition_penalty=1.0)
STAGE2_DEFAULTS = dict(max_new_tokens=512, do_sample=True, temperature=0.3, top_p=0.9, top_k=50,
                       repetition_penalty=1.8, length_penalty=1.2, num_beams=3)


def check_no_adapter(adapter_path):
    """The Stage-2 script loads a QLoRA adapter over a 4-bit base model (inference_vqa_stage2.py:120-150); the HIP
    path runs dense bf16 weights only -- the same refusal as Gemma3CausalLM.check_not_quantized."""
    if adapter_path:
        raise ValueError(QLORA_UNSUPPORTED)


def _pixels(images, vision, preprocessor):
    """Decoded images (uint8 [H, W, C] arrays or Pillow images) -> pixel_values, or a pixel tensor as it is."""
    if torch.is_tensor(images):
        return images.to(vision.device)
    if preprocessor is None:
        raise L.PtkError("inference: decoded images need an ImagePreprocessor (pass preprocessor=)")
    return preprocessor([np.asarray(im.convert("RGB") if hasattr(im, "convert") else im) for im in images])


def project_images(images, vision, projector, preprocessor=None) -> torch.Tensor:
    """[B, N - 1, H] f32: the projected patch embeddings of the scripts (last_hidden_state[:, 1:]).  The scripts
    run the projector module itself in bf16; here MLPProjector.forward keeps its own precision (fp32 parameters,
    bf16 GEMM operands, fp32 output, as under the trainer's autocast) and only the output is rounded to bf16 -- an
    approximation of the all-bf16 projector, not the same arithmetic."""
    patches = vision(_pixels(images, vision, preprocessor))[:, 1:, :]
    return projector.forward(patches).detach().to(torch.bfloat16).float().contiguous()


def embed_tokens(llm, ids) -> torch.Tensor:
    """`llm.get_input_embeddings()(ids)` of a bf16 Gemma3: bf16(E[id] * bf16(sqrt(hidden))), held in fp32."""
    E = llm.get_input_embeddings()
    scale = torch.tensor(math.sqrt(llm.cfg.hidden_size), dtype=torch.bfloat16, device=E.device)
    return (E[ids.to(E.device)] * scale).float()


def _decode(tokenizer, rows):
    return [tokenizer.decode(r, skip_special_tokens=True) for r in rows.cpu()]


def describe_images(images, vision, projector, llm, tokenizer, preprocessor=None, seed=0, **generation_args):
    """One generated description per image, from the image tokens alone (the Stage-1 alignment test)."""
    args = {**STAGE1_DEFAULTS, **generation_args}
    with torch.no_grad():
        prompt = project_images(images, vision, projector, preprocessor)
        out = llm.generate(prompt, pad_token_id=getattr(tokenizer, "pad_token_id", None),
                           eos_token_id=getattr(tokenizer, "eos_token_id", None), seed=seed, **args)
    return _decode(tokenizer, out)


def vqa_prompt(image, question, vision, projector, llm, tokenizer, preprocessor=None) -> torch.Tensor:
    """[1, N - 1 + Tq, H] f32: [projected patches | question embeddings] of one sample."""
    q = tokenizer(question, return_tensors="pt", add_special_tokens=False).input_ids
    images = image if torch.is_tensor(image) else [image]
    projected = project_images(images, vision, projector, preprocessor)
    return torch.cat([projected, embed_tokens(llm, q.to(torch.int64))], dim=1).contiguous()


def answer_question(image, question, vision, projector, llm, tokenizer, preprocessor=None, adapter_path=None, seed=0,
                    **generation_args):
    """The answer `process_sample` generates for one (image, question) sample."""
    check_no_adapter(adapter_path)
    args = {**STAGE2_DEFAULTS, **generation_args}
    beams = int(args.pop("num_beams"))
    pad, eos = getattr(tokenizer, "pad_token_id", None), getattr(tokenizer, "eos_token_id", None)
    with torch.no_grad():
        prompt = vqa_prompt(image, question, vision, projector, llm, tokenizer, preprocessor)
        if beams > 1:
            mask = torch.ones(prompt.shape[:2], dtype=torch.int32, device=prompt.device)
            out = llm.beam_generate(prompt, mask, num_beams=beams, eos_token_id=eos, pad_token_id=pad, seed=seed,
                                    **args)
        else:
            args.pop("length_penalty", None)   # (only beam search reads it)
            out = llm.generate(prompt, eos_token_id=eos, pad_token_id=pad, seed=seed, **args)
    return _decode(tokenizer, out)[0]
