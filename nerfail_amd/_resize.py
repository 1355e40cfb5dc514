"""The resize in front of the torchvision classifiers (GN:145-157, MD:110-113, MT:283-290), shared by gauss_net's cold tail and
model_test: torchvision if present (as the reference), else the same bilinear op in torch."""
import torch


def resize(x, size):
    try:
        from torchvision.transforms import Resize
        return Resize([size, size])(x)
    except ImportError:
        return torch.nn.functional.interpolate(x, size=(size, size), mode='bilinear', align_corners=False,
                                               antialias=True)
