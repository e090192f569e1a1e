"""Run by tests/test_gpu_hahog_adversarial.py in a fresh interpreter: images uploaded with torch, their ``data_ptr()`` handed to
``features.hahog_batch(shapes=...)`` (OSFM_HAHOG_IMAGE_ON_DEVICE), results equal to the host-image calls byte for byte and to the golden
record of the reference.  torch is imported and brings up its HIP runtime first; the library is loaded after it."""
import os
import sys

import numpy as np
import torch

torch.cuda.set_device(0)
torch.zeros(1, device="cuda").cpu()  # the runtime is up before the library is loaded

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import test_gpu_hahog_adversarial as t  # noqa: E402
from opensfm_amd import _lib  # noqa: E402

with np.load(t.GOLDEN) as g:
    golden = {k: g[k] for k in g.files}
count = [0]


def upload(im):
    x = torch.from_numpy(np.array(im)).to("cuda:0")
    torch.cuda.synchronize()  # the library reads the tensor on streams of its own
    assert x.is_contiguous() and x.numel() == im.size and x.element_size() == im.itemsize
    count[0] += 1
    return x.data_ptr(), x


t.check_resident_images(_lib.default_context(0), upload, lambda cid, p, d: t._check(golden, cid, p, d))
print("resident torch tensors OK: %d images" % count[0])
