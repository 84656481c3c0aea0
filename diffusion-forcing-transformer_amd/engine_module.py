"""The host base of the four backbone modules (UViT3DPose, UViT3D, DiT3D, DiT1D): one binding to an inference-engine family of
libdfot_hip.so and the plumbing around its handle -- the module tree built from the engine's dotted state-dict names, the weight sync,
the workspace reserve and the generation counter captured sampler graphs are checked against.

A subclass names its engine (``_family``: "uvit", "dit" or "dit1d"; ``_create``: which create entry point), fills ``self._ccfg`` and calls
``_build_tree()``.  Construction-time validation, initialisers, ``forward`` and everything about conditioning, taps and trainers are its own.
"""
from __future__ import annotations

import ctypes as C
import functools
from types import SimpleNamespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import capi

Layout = List[Tuple[str, Tuple[int, ...]]]


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default) if not hasattr(cfg, "get") else cfg.get(key, default)


class _Node(nn.Module):
    """Anonymous container so that dotted reference key names map onto a module tree."""


@functools.lru_cache(maxsize=None)
def engine_binding(family: str, create: str) -> SimpleNamespace:
    """the entry points of one engine family, looked up once; set_option is None where the family has none (dit1d)"""
    ops = ("destroy", "num_params", "param_name", "param_shape", "load_weight", "finalize", "reserve")
    return SimpleNamespace(create=getattr(capi.lib, create), set_option=getattr(capi.lib, f"dfot_{family}_set_option", None),
                           **{op: getattr(capi.lib, f"dfot_{family}_{op}") for op in ops})


class EngineModule(nn.Module):
    _family: str = ""
    _create: str = ""

    def __init__(self):
        super().__init__()
        self._handle = C.c_void_p()
        self._layout: Optional[Layout] = None
        self._names: List[str] = []
        self._synced: Optional[Tuple] = None
        self._reserved = 0
        self._op_key: Optional[int] = None
        self.reserve_generation = 0  # what a captured sampler graph is keyed to: see _bump_generation

    @property
    def _engine(self) -> SimpleNamespace:
        return engine_binding(self._family, self._create)

    # ------------------------------------------------------------------ handle and module tree
    def _ensure_handle(self) -> None:
        """Create the engine handle (device memory) from ``_ccfg`` unless it exists.  The engine's parameter list becomes the module's
        layout, or, where the module was built on the host from a layout of its own, has to equal it."""
        if self._handle.value:
            return
        eng, handle = self._engine, C.c_void_p()
        capi.check(eng.create(C.byref(self._ccfg), C.byref(handle)))
        shape, ndim = (C.c_int64 * 4)(), C.c_int()
        got = []
        for i in range(eng.num_params(handle)):
            capi.check(eng.param_shape(handle, i, shape, C.byref(ndim)))
            got.append((eng.param_name(handle, i).decode(), tuple(shape[k] for k in range(ndim.value))))
        if self._layout is not None and got != self._layout:
            eng.destroy(handle)
            raise RuntimeError("the engine's parameter list differs from the module's state-dict layout")
        self._handle, self._layout = handle, got

    def _build_tree(self, layout: Optional[Sequence] = None) -> None:
        """Register one tensor per state-dict key, in order.  ``layout`` None: the handle is created now and its list taken; given (the
        module is built on the host): the handle is created at the first weight sync or reserve and checked against it."""
        if layout is None:
            self._ensure_handle()
        else:
            self._layout = [(name, tuple(shape)) for name, shape in layout]
        self._names = [name for name, _ in self._layout]
        for name, shape in self._layout:
            *path, leaf = name.split(".")
            node: nn.Module = self
            for part in path:
                if part not in node._modules:
                    node.add_module(part, _Node())
                node = node._modules[part]
            t = self._new_tensor(name, shape)
            if isinstance(t, nn.Parameter):
                node.register_parameter(leaf, t)
            else:
                node.register_buffer(leaf, t, persistent=True)

    def _new_tensor(self, name: str, shape: Tuple[int, ...]) -> torch.Tensor:
        """what to register for this key: an nn.Parameter, or a plain tensor for a persistent buffer"""
        return nn.Parameter(torch.zeros(shape, dtype=torch.float32))

    def _tensors(self) -> Dict[str, torch.Tensor]:
        return dict(self.named_parameters())

    def _engine_tensors(self) -> Dict[str, torch.Tensor]:
        """everything the engine loads: the parameters and the persistent buffers"""
        return {**dict(self.named_parameters()), **dict(self.named_buffers())}

    # ------------------------------------------------------------------ weights -> engine, workspace
    def _bump_generation(self) -> None:
        """captured sampler graphs bake the kernels chosen for the old weights / options and the old workspace pointers: they are stale"""
        self.reserve_generation += 1

    def _signature(self) -> Tuple:
        return tuple((t.data_ptr(), t._version) for t in self._engine_tensors().values())

    def sync_weights(self, force: bool = False) -> None:
        sig = self._signature()
        if not force and sig == self._synced:
            return
        tensors = self._engine_tensors()
        for name in self._names:  # before a handle is created or anything is loaded
            if not tensors[name].is_cuda:
                raise RuntimeError(f"parameter {name} is on {tensors[name].device}; move the module to the GPU first")
        self._ensure_handle()
        eng, s = self._engine, capi.stream_ptr()
        for name in self._names:
            src = tensors[name].detach().to(torch.float32).contiguous()
            shape = (C.c_int64 * src.ndim)(*src.shape)
            capi.check(eng.load_weight(self._handle, name.encode(), capi.ptr(src), shape, src.ndim, s))
        capi.check(eng.finalize(self._handle, s))
        self._synced = sig
        self._bump_generation()

    def reserve(self, batch: int) -> None:
        if batch > self._reserved:
            torch.cuda.synchronize()
            self._ensure_handle()
            capi.check(self._engine.reserve(self._handle, int(batch)))
            self._reserved = batch
            self._bump_generation()
            self._after_reserve()

    def _after_reserve(self) -> None:
        """runs after the workspace has grown"""

    def set_option(self, key: str, value: int) -> None:
        self._bump_generation()  # options select kernels
        capi.check(self._engine.set_option(self._handle, key.encode(), int(value)))

    def __del__(self):
        try:
            if getattr(self, "_handle", None) and self._handle.value:
                self._engine.destroy(self._handle)
                self._handle = C.c_void_p()
        except Exception:
            pass
