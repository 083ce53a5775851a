"""MI355X-native adversarial training step of the Semantic-Pyramid GAN."""
from .ops import compute_dtype, set_compute_dtype  # noqa: F401
from .models import Discriminator, Generator, VGG16  # noqa: F401
from .lossfunction import (DiversityLoss, LSGANDiscriminatorLoss, LSGANGeneratorLoss,  # noqa: F401
                           SemanticReconstructionLoss, HingeDiscriminatorLoss, HingeGeneratorLoss,
                           LogisticDiscriminatorLoss, LogisticGeneratorLoss)
from .model_wrapper import ModelWrapper  # noqa: F401
from . import optim  # noqa: F401
