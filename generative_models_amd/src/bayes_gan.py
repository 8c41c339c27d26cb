"""Bayesian GAN (Saatchi & Wilson 2017; the reference's src/bayes_gan.py is a docstring and a TODO, its README to-do
list names it, README.md:95): Generator, Discriminator, BayesGAN and BayesGANTrainer with ns_gan.py's names and
layout -- state_dict keys G.<j>.linear/generate.*, D.<k>.linear/discriminate.*; compute runs on the gfx950 kernels
of generative_models_amd (SGHMC and the latent draws on the device Philox generator)."""
import _bootstrap  # noqa: F401
import numpy as np  # noqa: F401
import torch  # noqa: F401
import torch.nn as nn  # noqa: F401

from utils import *  # noqa: F401,F403
from generative_models_amd.bgan import BayesGAN, BayesGANTrainer, Discriminator, Generator  # noqa: F401
