"""Sliced-Wasserstein generator (Deshpande, Zhang & Schwing, arXiv 1803.11188; Kolouri et al., arXiv 1804.01947; Wu et
al., arXiv 1706.02631): Generator, SWG and SWGTrainer beside ns_gan.py, with its generator's names and layout --
state_dict keys G.linear.*, G.generate.*, so an NSGAN's or a GMMN's generator loads with strict=False -- trained without a
critic on the sliced squared 2-Wasserstein distance between a batch of samples and a batch of images; compute runs on the
gfx950 kernels of generative_models_amd (generative_models_amd/swg.py holds the contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.swg import SWG, SWGError, SWGTrainer, Generator  # noqa: F401
