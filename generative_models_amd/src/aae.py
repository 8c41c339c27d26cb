"""Adversarial autoencoder (the reference's README to-do list, README.md:95 "adversarial autoencoder"): Encoder,
Decoder, Discriminator, AAE and AAETrainer beside ae.py / vae.py, with their names and layout -- state_dict keys
encoder.linear/z.*, decoder.linear/recon.*, discriminator.linear/discriminate.*; compute runs on the gfx950 kernels
of generative_models_amd."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.aae import AAE, AAETrainer, Decoder, Discriminator, Encoder  # noqa: F401
