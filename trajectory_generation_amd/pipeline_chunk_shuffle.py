"""The module name the reference's training_indipendent_chunking.py imports: pipeline_indipendent_chunking under it."""
from .pipeline_indipendent_chunking import *  # noqa: F401,F403
