"""VQATrainerStage2's flag handling (Stage2/trainer.py:189-246), checked before any device work: the
constructor is given dummy towers on a machine without a GPU and must refuse from the flags alone."""
import pytest

from projectiontrainer_amd.vqa_trainer import VQATrainerStage2


def construct(**flags):
    kw = dict(freeze_vision_encoder=True, freeze_projection_layer=True, freeze_llm=False, enable_qlora=False,
              train_ve_first_epoch=False)
    kw.update(flags)
    # accelerator, vision_encoder, language_model, projection_layer, tokenizer, train_dataset, val_dataset,
    # output_dir, batch_size, learning_rate, weight_decay, num_epochs, gradient_accumulation_steps, warmup_ratio
    return VQATrainerStage2(None, object(), object(), object(), None, [], None, "unused", 2, 1e-3, 0.01, 1, 1, 0.05,
                            wandb_project="x", **kw)


def test_nothing_trainable_is_a_value_error():
    """freeze_llm and freeze_projection_layer together leave no parameter for the optimizer: the reference raises
    ValueError("No trainable parameters found. ...") at Stage2/trainer.py:242-243."""
    with pytest.raises(ValueError, match="No trainable parameters found"):
        construct(freeze_llm=True, freeze_projection_layer=True)


@pytest.mark.parametrize("flags", [dict(enable_qlora=True), dict(freeze_vision_encoder=False),
                                   dict(train_ve_first_epoch=True)],
                         ids=["enable_qlora", "unfrozen_vision_encoder", "train_ve_first_epoch"])
@pytest.mark.parametrize("proj", [True, False], ids=["proj_frozen", "proj_trained"])
def test_unsupported_flags_stay_not_implemented(flags, proj):
    with pytest.raises(NotImplementedError):
        construct(freeze_projection_layer=proj, **flags)
