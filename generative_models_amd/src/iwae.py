"""Importance-weighted autoencoder (Burda, Grosse & Salakhutdinov, arXiv 1509.00519): Encoder, Decoder, IWAE and
IWAETrainer beside vae.py, with its names and layout -- state_dict keys encoder.linear/mu/log_var.*,
decoder.linear/recon.*, so a VAE's weights load into an IWAE and back -- trained on the k-sample bound; compute runs on
the gfx950 kernels of generative_models_amd (generative_models_amd/iwae.py holds the contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.iwae import IWAE, IWAEError, IWAETrainer, Decoder, Encoder  # noqa: F401
