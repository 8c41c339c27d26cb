"""Denoising diffusion probabilistic model (Ho, Jain & Abbeel, arXiv 2006.11239) with the generalised sampler of Song,
Meng & Ermon (arXiv 2010.02502): Denoiser, DDPM and DDPMTrainer in the collection's layout -- state_dict keys
denoiser.linear/hidden/out.* -- trained on L_simple and sampled on the gfx950 kernels of generative_models_amd
(generative_models_amd/ddpm.py holds the contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.ddpm import DDPM, DDPMError, DDPMTrainer, Denoiser  # noqa: F401
