"""Training entry point of the SE-ResNet-unrolled cine reconstruction on MI355X:
the reference's scripts/train_se.py by name.  The trainer is scripts/train_swin.py
(same command line and training semantics); its build_model maps MODEL_TYPE 'SE'
(configs/config_se.yaml) to dl_cs.models.unrolledSE.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from train_swin import build_model, create_arg_parser, main  # noqa: E402,F401

if __name__ == "__main__":
    main()
