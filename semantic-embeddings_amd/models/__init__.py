"""PyTorch-ROCm backbones behind ``utils.build_network`` (the reference's models/ factory)."""
from . import cifar_pyramidnet, cifar_resnet, plainnet, resnet50  # noqa: F401
