"""DeBERTa-v3 dropout, the parts that need no GPU: the --text_dropout flag and where build_encoders
sends it (a trainable DeBERTa-v3 gets both probabilities; a frozen one and BERT ignore it with a warning),
the shared seed mixin, and the binding's host-side surface."""
import warnings

import pytest

VIT = ["--image_encoder", "google/vit-base-patch16-224"]


def test_text_dropout_flag_parses():
    from mmfd.train import parse_args
    assert parse_args([]).text_dropout == 0.0
    assert parse_args(["--text_dropout", "0.1"]).text_dropout == pytest.approx(0.1)
    a = parse_args(["--train_text_encoder", "--text_dropout", "0.25"])
    assert a.train_text_encoder is True and a.text_dropout == pytest.approx(0.25)
    with pytest.raises(SystemExit):
        parse_args(["--text_dropout", "much"])


def test_build_encoders_sends_text_dropout_to_a_trainable_deberta():
    from mmfd.deberta import DebertaV2Model
    from mmfd.train import build_encoders, parse_args
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # no warning on the supported path
        text, _, frozen, _ = build_encoders(parse_args(VIT + ["--train_text_encoder", "--text_dropout", "0.1"]), "cpu")
        assert isinstance(text, DebertaV2Model) and text.config.trainable and frozen is False
        assert text.config.hidden_dropout_prob == pytest.approx(0.1)
        assert text.config.attention_probs_dropout_prob == pytest.approx(0.1)
        # the default leaves the model as it was: trainable, both probabilities 0
        text, _, frozen, _ = build_encoders(parse_args(VIT + ["--train_text_encoder"]), "cpu")
        assert text.config.trainable and text.config.hidden_dropout_prob == 0.0
        assert text.config.attention_probs_dropout_prob == 0.0


@pytest.mark.parametrize("extra", [[], ["--train_text_encoder", "--freeze_text"]])
def test_frozen_deberta_ignores_text_dropout_with_a_warning(extra):
    from mmfd.train import build_encoders, parse_args
    with pytest.warns(UserWarning, match="text_dropout is ignored"):
        text, _, frozen, _ = build_encoders(parse_args(VIT + extra + ["--text_dropout", "0.1"]), "cpu")
    assert frozen is True and not text.config.trainable
    assert text.config.hidden_dropout_prob == 0.0 and text.config.attention_probs_dropout_prob == 0.0


def test_bert_ignores_text_dropout_with_a_warning():
    from mmfd.encoders import BertConfig, BertModel
    from mmfd.train import build_encoders, parse_args
    args = parse_args(VIT + ["--text_encoder", "bert-base-uncased", "--text_dropout", "0.3"])
    with pytest.warns(UserWarning, match="text_dropout is ignored"):
        text, _, _, _ = build_encoders(args, "cpu")
    assert isinstance(text, BertModel)
    assert text.config.hidden_dropout_prob == BertConfig().hidden_dropout_prob == 0.1
    assert text.config.attention_probs_dropout_prob == 0.1


def test_text_dropout_out_of_range_is_refused():
    from mmfd.train import build_encoders, parse_args
    with pytest.raises(ValueError, match="text_dropout"):
        build_encoders(parse_args(VIT + ["--train_text_encoder", "--text_dropout", "1.0"]), "cpu")


def test_seed_code_is_shared_with_bert():
    from mmfd import blocks as Bk
    from mmfd.deberta import DebertaV2Model
    from mmfd.encoders import BertModel
    for cls in (BertModel, DebertaV2Model):
        assert issubclass(cls, Bk.StepSeeded)
        assert cls.manual_seed is Bk.StepSeeded.manual_seed and cls._fork_seed is Bk.StepSeeded._fork_seed
    m = DebertaV2Model(vocab_size=50, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64)
    assert m.manual_seed(77) is m and m._seed_value == 77 and m._seed is None  # the device seed is made on first use


def test_binding_is_declared():
    from mmfd import kernels as K
    assert "mmfd_attn_bwd_ds" in K.SIGNATURES
    assert callable(K.attn_bwd_ds)


@pytest.mark.parametrize("dtype,D,p,name", [("f32", 64, 0.0, "attn_bwd_ds_kernel<float,64>"),
                                            ("f32", 64, 0.1, "attn_bwd_ds_kernel<float,64,1>"),
                                            ("bf16", 16, 0.1, "attn_bwd_ds_kernel<bf16,32,1>"),
                                            ("bf16", 48, 0.0, "attn_bwd_ds_kernel<bf16,64>")])
def test_plan_export_of_the_ds_entry(dtype, D, p, name):
    """mmfd_debug_attn_plan(bwd = 2): one launch of the dS kernel over 64-query blocks, the dropout-free
    instantiation under the name it has in mmfd_attn_bwd's plans, and the host refusals without a launch"""
    from tests.attn_cases import plan_lines
    from tests.test_attn_plan_cpu import attn_args
    from mmfd import kernels as K
    a = attn_args(1, dtype, 2, 3, 130, 65, D, key_bias=1, rel_bias="batch", p=p, d_rel_bias=1)
    lines = plan_lines(a, 2, "split")
    assert lines[0] == "family=stream" and len(lines) == 2
    lds = 2 * 64 * (64 if D > 32 else 32) * (4 if dtype == "f32" else 2)
    assert lines[1].startswith(f"{name} grid=3,6,1 block=256 lds={lds}"), lines
    # the same arguments, backward plan: mmfd_attn_bwd's own d_rel_bias launch is unchanged (and refuses dropout)
    if p == 0.0:
        assert plan_lines(a, 1, "split")[-1].startswith(name + " ")
    lib = K.load()
    import ctypes
    buf = ctypes.create_string_buffer(1024)
    for kw, msg in ((dict(rel_bias="shared"), "per-batch rel_bias"), (dict(rel_bias="batch", rb_mod=2), "per-batch rel_bias")):
        bad = attn_args(1, dtype, 2, 3, 130, 65, D, p=p, d_rel_bias=1, **kw)
        assert lib.mmfd_debug_attn_plan(ctypes.byref(bad), 2, buf, len(buf)) != 0
        assert msg in lib.mmfd_last_error_string().decode()
    alias = attn_args(1, dtype, 2, 3, 130, 65, D, rel_bias="batch", p=p, d_rel_bias=1)
    alias.d_rel_bias = alias.rel_bias
    assert lib.mmfd_debug_attn_plan(ctypes.byref(alias), 2, buf, len(buf)) != 0
    assert "alias" in lib.mmfd_last_error_string().decode()
