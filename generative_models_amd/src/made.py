"""Masked autoencoder for distribution estimation (Germain, Gregor, Murray & Larochelle, arXiv 1502.03509): MADE and
MADETrainer in the collection's layout -- state_dict keys linear.* / out.* and the degree buffers m_in / m_h -- trained on
its exact negative log-likelihood and sampled in one launch on the gfx950 kernels of generative_models_amd
(generative_models_amd/made.py holds the contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.made import MADE, MADEError, MADETrainer  # noqa: F401
