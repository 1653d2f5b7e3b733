"""a handle with a rack in the host emulation: now part of emu.py"""
from .emu import ANCHOR, RackCapture, rack_info, reset_rack, reset_to_rack, set_rack, step_rack  # noqa: F401
