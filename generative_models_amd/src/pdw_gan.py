"""Primal-Dual Wasserstein GAN (the reference's README to-do list, README.md:95 "Primal-Dual Wasserstein GAN"; Gemici,
Akata, Welling, arXiv 1805.09575): PDWGAN and PDWGANTrainer beside w_gp_gan.py / aae.py, with their names and layout --
state_dict keys E.linear/z.*, G.linear/generate.*, D.linear/discriminate.*; compute runs on the gfx950 kernels of
generative_models_amd."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.aae import Encoder  # noqa: F401
from generative_models_amd.trainers import CriticReLU as Discriminator, Generator  # noqa: F401
from generative_models_amd.pdwgan import PDWGAN, PDWGANTrainer  # noqa: F401
