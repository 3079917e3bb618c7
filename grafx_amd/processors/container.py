"""Processor containers (mirrors grafx.processors.container — reference container.py:10-299).
Pure composition: they call the wrapped (HIP) processors and combine their outputs with a few
elementwise torch ops; no kernels of their own."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .core._buffer_io import StreamIO, child_stream
from .core.utils import rms_difference


def _split(out):
    return out if isinstance(out, tuple) else (out, None)


class _Container(StreamIO):
    """The block protocol of a container: its carry is the tuple of its children's carries, in their order."""

    def _children(self):
        return [self.processor] if hasattr(self, "processor") else list(self.processors.values())

    def stream_check(self):
        for proc in self._children():
            child_stream(proc, self).stream_check()

    def stream_silence(self, carry):
        """Child by child: every wrapped processor says what its own silence is."""
        if carry is None:
            return None
        return tuple(child_stream(proc, self).stream_silence(c) for proc, c in zip(self._children(), carry))


class DryWet(_Container, nn.Module):
    """y = w * processor(x) + (1 - w) * x (container.py:10-82)."""

    def __init__(self, processor, external_param=True):
        super().__init__()
        self.processor = processor
        self.external_param = external_param

    def forward(self, input_signals, drywet_weight, **processor_kwargs):
        wet, extra = _split(self.processor(input_signals, **processor_kwargs))
        w = drywet_weight.view(-1, 1, 1)
        mixed = w * wet + (1 - w) * input_signals
        return mixed if extra is None else (mixed, extra)

    def stream_block(self, x4, out4, carry, drywet_weight, **processor_kwargs):
        wet = torch.empty_like(out4, memory_format=torch.contiguous_format)
        carry = child_stream(self.processor, self).stream_block(x4, wet, None if carry is None else carry[0],
                                                                **processor_kwargs)
        w = drywet_weight.view(*x4.shape[:2], 1, 1)
        torch.add(w * wet, (1 - w) * x4, out=out4)
        return (carry,)

    def parameter_size(self):
        size = self.processor.parameter_size()
        if not self.external_param:
            size["drywet_weight"] = (1,)
        return size


class SerialChain(_Container, nn.Module):
    """Processors applied one after another; parameters are a dict keyed like the processors (85-148)."""

    def __init__(self, processors):
        super().__init__()
        self.processors = nn.ModuleDict(processors)

    def forward(self, input_signals, **processors_kwargs):
        signal, intermediates = input_signals, {}
        for name, proc in self.processors.items():
            signal, extra = _split(proc(signal, **processors_kwargs[name]))
            if extra is not None:
                intermediates[name] = extra
        return signal, intermediates

    def stream_block(self, x4, out4, carry, **processors_kwargs):
        signal, carries, last = x4, [], len(self.processors) - 1
        for i, (name, proc) in enumerate(self.processors.items()):
            dest = out4 if i == last else torch.empty_like(out4, memory_format=torch.contiguous_format)
            carries.append(child_stream(proc, self).stream_block(signal, dest, None if carry is None else carry[i],
                                                                 **processors_kwargs[name]))
            signal = dest
        return tuple(carries)

    def parameter_size(self):
        return {k: v.parameter_size() for k, v in self.processors.items()}


class ParallelMix(_Container, nn.Module):
    """Weighted sum of processors fed the same input (151-222)."""

    def __init__(self, processors, activation="softmax"):
        super().__init__()
        self.processors = nn.ModuleDict(processors)
        if activation not in ("softmax", "softplus"):
            raise ValueError(f"Unsupported activation: {activation}")
        self.activation = activation
        self.mult = 1 / (math.log(2) * len(self.processors))

    def get_weight(self, weights):
        if self.activation == "softmax":
            return torch.softmax(weights, dim=-1)
        return F.softplus(weights) * self.mult

    def forward(self, input_signals, parallel_weights, **processors_kwargs):
        weights = self.get_weight(parallel_weights)
        total, intermediates = None, {}
        for i, (name, proc) in enumerate(self.processors.items()):
            out, extra = _split(proc(input_signals, **processors_kwargs[name]))
            if extra is not None:
                intermediates[name] = extra
            out = out * weights[..., i, None, None]
            total = out if total is None else total + out
        return total, intermediates

    def stream_block(self, x4, out4, carry, parallel_weights, **processors_kwargs):
        weights = self.get_weight(parallel_weights).view(*x4.shape[:2], -1)
        total, carries = None, []
        for i, (name, proc) in enumerate(self.processors.items()):
            branch = torch.empty_like(out4, memory_format=torch.contiguous_format)
            carries.append(child_stream(proc, self).stream_block(x4, branch, None if carry is None else carry[i],
                                                                 **processors_kwargs[name]))
            branch = branch * weights[..., i, None, None]
            total = branch if total is None else total + branch
        out4.copy_(total)
        return tuple(carries)

    def parameter_size(self):
        size = {k: v.parameter_size() for k, v in self.processors.items()}
        size["parallel_weights"] = len(self.processors)
        return size


class GainStagingRegularization(_Container, nn.Module):
    """Adds the input/output log-RMS difference to the intermediates (231-299)."""

    def __init__(self, processor, key="gain_reg"):
        super().__init__()
        self.processor = processor
        self.key = key

    def forward(self, input_signals, **processor_kwargs):
        out, extra = _split(self.processor(input_signals, **processor_kwargs))
        extra = {} if extra is None else extra
        assert self.key not in extra
        extra[self.key] = rms_difference(input_signals, out)
        return out, extra

    def stream_block(self, x4, out4, carry, **processor_kwargs):
        """The regulariser is a by-product of the signal path: a streamed block renders the wrapped processor alone."""
        return (child_stream(self.processor, self).stream_block(x4, out4, None if carry is None else carry[0],
                                                                **processor_kwargs),)

    def parameter_size(self):
        return self.processor.parameter_size()
