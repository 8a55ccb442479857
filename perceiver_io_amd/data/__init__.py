"""Data modules: IMDB (text), MNIST (images), synthetic ImageNet-shape images, pre-decoded ``.npy`` images,
LArTPC-shape events; ``DeviceAugment`` draws the parameters of the device-side image augmentation."""
from .augment import DeviceAugment, RandAugment
from .imdb import Collator, IMDBDataModule, IMDBDataset, load_split
from .mnist import MNISTDataModule, NpyImageDataModule, SyntheticImageDataModule
from .registry import DATAMODULE_REGISTRY, register_datamodule
from .synthetic import SyntheticImages, SyntheticLArTPC, SyntheticText, lartpc_event

__all__ = ["Collator", "IMDBDataModule", "IMDBDataset", "load_split", "MNISTDataModule", "SyntheticImageDataModule",
           "NpyImageDataModule", "DeviceAugment", "RandAugment",
           "DATAMODULE_REGISTRY", "register_datamodule", "SyntheticImages", "SyntheticLArTPC", "SyntheticText",
           "lartpc_event"]
