"""Binary restricted Boltzmann machine (Smolensky 1986; Hinton 2002; Tieleman 2008): RBM and RBMTrainer in the
collection's layout -- state_dict keys linear.* and vbias -- trained by contrastive divergence (CD-k or persistent CD),
sampled and scored by annealed importance sampling in one launch each on the gfx950 kernels of generative_models_amd
(generative_models_amd/rbm.py holds the contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.rbm import RBM, RBMError, RBMTrainer  # noqa: F401
