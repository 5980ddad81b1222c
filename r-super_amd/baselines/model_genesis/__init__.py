"""Models Genesis self-supervised pre-training (rsuper_train/baselines/model_genesis of the reference): the pretext pairs on the device."""
from .utils import (GenesisPlan, bezier_curve, generate_one_pair, generate_pair_batch, genesis_launches, make_genesis_plan,  # noqa: F401
                    plan_genesis_pair)
