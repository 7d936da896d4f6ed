"""Image files in: mmfd.preprocess.ImagePreprocessor("blip") against transformers' BlipImageProcessorPil bit for
bit (PIL's bicubic resize, the 1/255 rescale, CLIP mean / std), and Captioner on PIL images."""
import numpy as np
import pytest
import torch

from tests import blip_refs as R
from tests.test_beam_cpu import SIZES, random_image

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hf(images, S):
    from transformers import BlipImageProcessorPil
    return BlipImageProcessorPil(size={"height": S, "width": S})(images=images, return_tensors="pt")["pixel_values"]


@pytest.mark.parametrize("S", [16, 48])
def test_blip_mode_is_bit_equal_to_transformers(S):
    from PIL import Image
    from mmfd.preprocess import ImagePreprocessor
    images = [Image.fromarray(random_image(h, w, seed=h + w)) for (h, w), _ in SIZES]
    got = ImagePreprocessor("blip", device=DEV, size=S)(images)
    ref = _hf(images, S)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(images), 3, S, S)
    assert torch.equal(got.cpu(), ref)


def test_blip_mode_default_size_on_a_photo_sized_image():
    from PIL import Image
    from mmfd.preprocess import ImagePreprocessor
    img = Image.fromarray(random_image(480, 640, seed=1))
    pre = ImagePreprocessor("blip", device=DEV)
    assert pre.out_hw == (384, 384)
    assert torch.equal(pre([img]).cpu(), _hf([img], 384))
    arr = np.asarray(img)
    assert torch.equal(pre([arr]).cpu(), _hf([img], 384))  # a uint8 HWC array is the same image


def test_captioner_takes_pil_images():
    from PIL import Image
    from mmfd.blip import BlipConfig, BlipForConditionalGeneration
    from mmfd.caption import Captioner
    from tests.toy_tokenizer import toy_tokenizer
    z, cfg, W = R.load_fixture()
    m = BlipForConditionalGeneration(BlipConfig(vision=cfg["vision"], text=cfg["text"]))
    m.load_state_dict(W, strict=True)
    for p in m.parameters():
        p.requires_grad_(False)
    m = m.to(DEV).eval()
    S = cfg["vision"]["image_size"]
    images = [Image.fromarray(random_image(h, w, seed=7 * h + w)) for h, w in ((97, 61), (33, 47), (120, 160))]
    px = _hf(images, S)
    for nb in (1, 3):
        cap = Captioner(m, tokenizer=toy_tokenizer(), use_graph=False, num_beams=nb)
        assert torch.equal(cap.pixels(images).cpu(), px)
        ids = cap.generate_ids(images)
        assert ids.shape[0] == 3 and torch.equal(ids, cap.generate_ids(px))
        one = cap.generate_ids(images[0])  # a single PIL image is a batch of one
        assert one.shape[0] == 1 and torch.equal(one[0], ids[0, :one.shape[1]])
        texts = cap.caption(images)
        assert texts == cap.caption(px) and len(texts) == 3 and all(isinstance(t, str) for t in texts)
