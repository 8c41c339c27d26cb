"""beta-TCVAE (Chen et al., arXiv 1802.04942): Encoder, Decoder, TCVAE and TCVAETrainer beside vae.py, with its names
and layout -- state_dict keys encoder.linear/mu/log_var.*, decoder.linear/recon.*, so a VAE's or an IWAE's weights load
-- trained on the ELBO with its KL term split into mutual information, total correlation and dimension-wise KL under
the weights alpha, beta, gamma (all equal: the beta-VAE); compute runs on the gfx950 kernels of generative_models_amd
(generative_models_amd/tcvae.py holds the contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.tcvae import TCVAE, TCVAEError, TCVAETrainer, Decoder, Encoder  # noqa: F401
