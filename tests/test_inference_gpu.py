"""The reference's two inference calls (projectiontrainer_amd/inference.py) on the `tiny` preset with a stub
tokenizer: describe_images (Stage1/inference_stage1.py:150-193 -- the projected patches alone as the prompt) and
answer_question (process_sample, Stage2/inference_vqa_stage2.py:211-281 -- [projected | question embeddings], beam
search with the script's repetition_penalty 1.8 and length_penalty 1.2)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class Tok:
    """Words "w<id>" <-> token ids; ids 0 (pad) and 1 (eos) are the special tokens."""
    pad_token_id, eos_token_id = 0, 1

    def __call__(self, text, return_tensors="pt", add_special_tokens=True):
        ids = [int(w[1:]) for w in text.split()]
        if add_special_tokens:
            ids = [2] + ids   # (a BOS the Stage-2 script must not get)
        return types.SimpleNamespace(input_ids=torch.tensor([ids], dtype=torch.int64))

    def decode(self, seq, skip_special_tokens=True):
        return " ".join(f"w{int(t)}" for t in np.asarray(seq) if not (skip_special_tokens and int(t) in (0, 1)))


@pytest.fixture(scope="module")
def towers(gpu):
    from projectiontrainer_amd import weights as W
    from projectiontrainer_amd.config import PRESETS
    from projectiontrainer_amd.data import ImagePreprocessor
    from projectiontrainer_amd.gemma3 import Gemma3CausalLM
    from projectiontrainer_amd.projectors import MLPProjector
    from projectiontrainer_amd.siglip import SiglipVisionTower
    cfg = PRESETS["tiny"]
    proj = MLPProjector(cfg.vision.hidden_size, cfg.text.hidden_size, device=gpu)
    proj.load_state_dict({k: torch.from_numpy(v)
                          for k, v in W.projector_params(cfg.vision.hidden_size, cfg.text.hidden_size).items()})
    vision = SiglipVisionTower(cfg.vision, W.siglip_vision_params(cfg.vision), gpu)
    llm = Gemma3CausalLM(cfg.text, W.gemma3_params(cfg.text), gpu, max_pos=256)
    rng = np.random.default_rng(3)
    images = [rng.integers(0, 256, (40, 56, 3), dtype=np.uint8), rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)]
    return cfg, vision, proj, llm, ImagePreprocessor(cfg.vision.image_size, gpu), images


def test_describe_images_returns_one_text_per_image(gpu, towers):
    from projectiontrainer_amd import inference as I
    cfg, vision, proj, llm, pre, images = towers
    out = I.describe_images(images, vision, proj, llm, Tok(), preprocessor=pre, seed=5, max_new_tokens=6)
    assert len(out) == 2 and all(isinstance(s, str) for s in out)
    assert all(len(s.split()) <= 6 and all(w.startswith("w") for w in s.split()) for s in out)
    assert out == I.describe_images(images, vision, proj, llm, Tok(), preprocessor=pre, seed=5, max_new_tokens=6)
    # the script's repetition_penalty reaches generate
    pen = I.describe_images(images, vision, proj, llm, Tok(), preprocessor=pre, seed=5, max_new_tokens=6,
                            do_sample=False, repetition_penalty=1.8)
    ids = [[int(w[1:]) for w in s.split()] for s in pen]
    prompt = I.project_images(images, vision, proj, pre)
    want = llm.generate(prompt, max_new_tokens=6, do_sample=False, repetition_penalty=1.8, pad_token_id=0,
                        eos_token_id=1).cpu()
    assert ids == [[int(t) for t in r if int(t) not in (0, 1)] for r in want]


def test_answer_question_is_beam_generate_on_the_scripts_prompt(gpu, towers):
    """num_beams 3, repetition_penalty 1.8, length_penalty 1.2 (the script's defaults): deterministic for a seed,
    and exactly what beam_generate returns for the prompt built by hand -- the projected patches without the
    first token, then bf16(E[q] * bf16(sqrt H)) of the question tokenised WITHOUT special tokens, mask all ones."""
    from projectiontrainer_amd import inference as I
    cfg, vision, proj, llm, pre, images = towers
    tok, q = Tok(), "w17 w5 w301 w44"
    a = I.answer_question(images[0], q, vision, proj, llm, tok, preprocessor=pre, seed=9, max_new_tokens=8)
    b = I.answer_question(images[0], q, vision, proj, llm, tok, preprocessor=pre, seed=9, max_new_tokens=8)
    assert isinstance(a, str) and a == b
    patches = vision(pre([images[0]]))[:, 1:, :]
    projected = proj.forward(patches).detach().to(torch.bfloat16).float()
    ids = torch.tensor([[17, 5, 301, 44]], device=gpu)
    scale = torch.tensor(cfg.text.hidden_size ** 0.5, dtype=torch.bfloat16, device=gpu)
    qe = (llm.get_input_embeddings()[ids] * scale).float()
    prompt = torch.cat([projected, qe], 1).contiguous()
    assert prompt.shape[1] == cfg.vision.num_patches - 1 + 4
    mask = torch.ones(prompt.shape[:2], dtype=torch.int32, device=gpu)
    want = llm.beam_generate(prompt, mask, num_beams=3, max_new_tokens=8, do_sample=True, temperature=0.3, top_p=0.9,
                             top_k=50, repetition_penalty=1.8, length_penalty=1.2, eos_token_id=1, pad_token_id=0,
                             seed=9)
    assert a == tok.decode(want[0].cpu())
    # num_beams 1 goes through generate with the same penalty
    one = I.answer_question(images[0], q, vision, proj, llm, tok, preprocessor=pre, seed=9, max_new_tokens=8,
                            num_beams=1)
    w1 = llm.generate(prompt, max_new_tokens=8, do_sample=True, temperature=0.3, top_p=0.9, top_k=50,
                      repetition_penalty=1.8, eos_token_id=1, pad_token_id=0, seed=9)
    assert one == tok.decode(w1[0].cpu())


def test_answer_question_refuses_an_adapter(gpu, towers):
    from projectiontrainer_amd import inference as I
    cfg, vision, proj, llm, pre, images = towers
    with pytest.raises(ValueError, match="QLoRA"):
        I.answer_question(images[0], "w3", vision, proj, llm, Tok(), preprocessor=pre, adapter_path="adapters/x")
