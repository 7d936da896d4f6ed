"""The three LM-head products of mmfd.blip's caption loss at BLIP's real vocabulary, asked of mmfd_gemm's launch
plan (host arithmetic: no GPU). 30,524 = 4 * 7631 is no multiple of 8: a dense bf16 [R, 30524] dlogits would send
dG = dlogits W (K = V contiguous) and dW = dlogits^T G (M = V contiguous) to the one-output-per-thread kernel, so
the loss path lays the vocabulary out in vocab_ld(V) columns / rows."""
import pytest
import torch

R, V, E = 20 * 21, 30524, 768  # tools/caption_bench.py --loss: B = 20, T = 21, blip-image-captioning-large


def test_vocab_ld():
    from mmfd.blip import vocab_ld
    assert [vocab_ld(v) for v in (1, 8, 200, 203, 30522, 30524)] == [8, 8, 200, 208, 30528, 30528]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("rows", [R, 16, 32 * 40])
def test_lm_head_products_run_on_mfma_kernels(dtype, rows):
    from mmfd.blip import lm_head_gemm_paths
    paths = lm_head_gemm_paths(dtype, rows, V, E)
    print(dtype, rows, paths)
    assert set(paths) == {"logits", "dG", "dW"}
    for name, (path, kernel) in paths.items():
        assert path is not None and path not in ("simple", "empty"), (name, path, kernel)


def test_the_unpadded_bf16_products_would_not():
    """why the padding is there: the same two backward products on a dense [R, 30524] bf16 dlogits"""
    from mmfd import kernels as K
    assert K.gemm_path(torch.bfloat16, R, E, V, trans_b=True)[0] == "simple"
    assert K.gemm_path(torch.bfloat16, V, E, R, trans_a=True, trans_b=True, out_dtype=torch.float32, a_rowsum=True)[0] == "simple"
