"""Denoising VAE (the reference's README to-do list, "denoising VAE"): Encoder, Decoder, DVAE and DVAETrainer beside
vae.py, with its names and layout -- state_dict keys encoder.linear/mu/log_var.*, decoder.linear/recon.*, so a DVAE's
weights load into a VAE and back -- and corrupt(), the device corruption the trainer feeds the encoder; compute runs on
the gfx950 kernels of generative_models_amd."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.dvae import DVAE, DVAETrainer, Decoder, Encoder, NoiseError, corrupt  # noqa: F401
