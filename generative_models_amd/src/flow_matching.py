"""Flow matching / rectified flow (Lipman et al., arXiv 2210.02747; Liu, Gong & Liu, arXiv 2209.03003): VelocityField,
FlowMatching and FlowMatchingTrainer in the collection's layout -- state_dict keys field.linear/hidden/out.* -- a
continuous normalizing flow trained by velocity regression, sampled by euler / heun / rk4 and scored with the exact
divergence of its field on the gfx950 kernels of generative_models_amd (generative_models_amd/flowmatch.py holds the
contract)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.flowmatch import FlowMatchError, FlowMatching, VelocityField  # noqa: F401
from generative_models_amd.flowmatch import FlowMatchTrainer as FlowMatchingTrainer  # noqa: F401
