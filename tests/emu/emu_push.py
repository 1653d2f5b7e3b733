"""external pushes in the host emulation: now part of emu.py"""
from .emu import push_rows, step_push  # noqa: F401
