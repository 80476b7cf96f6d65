"""Child process of tests/test_hip_encoder_train.py: a process-fresh SpatialEncoder with trunk = "hip_train", loaded from a
state_dict file, runs one forward + backward in training mode on the images of a file with the cotangents of a file and writes
the levels, every gradient and every buffer.
usage: encoder_train_child.py <state_dict.pt> <images.pt> <cotangents.pt> <out.pt>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pixelnerf_amd.model.encoder import SpatialEncoder  # noqa: E402


def run(enc, images, cotangents):
    """one forward + backward of the trunk -> {name: cpu tensor} of the levels, the gradients and the buffers"""
    x = images.detach().clone().requires_grad_(True)
    levels = enc._stages(x)
    params = [p for p in enc.model.parameters()]
    loss = sum((t * g).sum() for t, g in zip(levels, cotangents))
    grads = torch.autograd.grad(loss, [x] + params, allow_unused=True)
    out = {f"level{i}": t.detach().cpu() for i, t in enumerate(levels)}
    out["grad.image"] = grads[0].cpu()
    for (name, _), g in zip(enc.model.named_parameters(), grads[1:]):
        if g is not None:
            out["grad." + name] = g.cpu()
    for name, b in enc.model.named_buffers():
        out["buffer." + name] = b.detach().cpu().clone()
    return out


def main(state_path, images_path, cot_path, out_path):
    enc = SpatialEncoder("resnet18", pretrained=False, num_layers=4, use_first_pool=True)
    enc.load_state_dict(torch.load(state_path, map_location="cpu"))
    enc.trunk = "hip_train"
    enc = enc.to("cuda:0").train()
    images = torch.load(images_path, map_location="cpu").to("cuda:0")
    cot = [g.to("cuda:0") for g in torch.load(cot_path, map_location="cpu")]
    torch.save(run(enc, images, cot), out_path)


if __name__ == "__main__":
    main(*sys.argv[1:5])
