"""Generative moment matching network (Li, Swersky & Zemel, arXiv 1502.02761; Dziugaite, Roy & Ghahramani, arXiv
1505.03906): Generator, GMMN and GMMNTrainer beside ns_gan.py, with its generator's names and layout -- state_dict keys
G.linear.*, G.generate.*, so an NSGAN's generator loads with strict=False -- trained without a critic on the kernel
maximum mean discrepancy between a batch of samples and a batch of images; compute runs on the gfx950 kernels of
generative_models_amd (generative_models_amd/gmmn.py holds the contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.gmmn import GMMN, GMMNError, GMMNTrainer, Generator  # noqa: F401
