"""Spectrally normalised hinge GAN (spectral normalisation: Miyato et al. 2018, arXiv 1802.05957; hinge loss, two
learning rates and Adam betas (0, 0.9): Zhang et al. 2018, arXiv 1805.08318): Generator, Discriminator, SNGAN and
SNGANTrainer beside ns_gan.py, with its names and loop -- state_dict keys G.linear/generate.*, D.linear/discriminate.*
and D.u; compute runs on the gfx950 kernels of generative_models_amd."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.sngan import SNGAN, SNGANTrainer, Discriminator, Generator  # noqa: F401
