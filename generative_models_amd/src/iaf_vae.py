"""Inverse autoregressive flow VAE (Kingma et al., arXiv 1606.04934): Encoder, Decoder, IAFVAE and IAFVAETrainer beside
vae.py, with its names and layout -- state_dict keys encoder.linear/mu/log_var.*, decoder.linear/recon.* plus
encoder.context.* and flow.W1 / flow.U / flow.b1 / flow.W2 / flow.b2 / flow.m_in, so a VAE's weights load with
strict=False -- K masked inverse-autoregressive layers on the encoder's Gaussian, trained on the k-sample bound; compute
runs on the gfx950 kernels of generative_models_amd (generative_models_amd/iafvae.py holds the contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.iafvae import IAFVAE, IAFVAEError, IAFVAETrainer, Decoder, Encoder  # noqa: F401
