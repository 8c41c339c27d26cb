"""Class-conditional VAE (the reference's README to-do list, README.md:95 "Models: CVAE"): Encoder, Decoder, CVAE and
CVAETrainer beside vae.py, with its names and layout -- state_dict keys encoder.linear/label/mu/log_var.*,
decoder.linear/label/recon.* (the `label` layers have no bias); compute runs on the gfx950 kernels of
generative_models_amd."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.cvae import CVAE, CVAETrainer, Decoder, Encoder, LabelError  # noqa: F401
