"""Child process of tests/test_hip_encoder_trunk.py: a process-fresh SpatialEncoder with trunk = "hip", loaded from a state_dict
file, encodes the images of a file and writes the latent.  usage: encoder_trunk_child.py <state_dict.pt> <images.pt> <latent_out.pt>"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pixelnerf_amd.model.encoder import SpatialEncoder  # noqa: E402


def main(state_path, images_path, out_path):
    enc = SpatialEncoder("resnet34", pretrained=False, num_layers=4, use_first_pool=False)
    enc.load_state_dict(torch.load(state_path, map_location="cpu"))
    enc.trunk = "hip"
    enc = enc.to("cuda:0").eval()
    with torch.no_grad():
        latent = enc(torch.load(images_path, map_location="cpu").to("cuda:0"))
    torch.save(latent.cpu(), out_path)


if __name__ == "__main__":
    main(*sys.argv[1:4])
