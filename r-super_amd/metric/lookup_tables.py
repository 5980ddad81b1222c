"""rsuper_train/metric/lookup_tables.py: the neighbourhood encoding and the resolution of the surfel area table.

ENCODE_NEIGHBOURHOOD_3D_KERNEL is the eight powers of two that turn a 2x2x2 voxel neighbourhood into a code 0..255.  The area of the surfel of
each code comes from the reference's 256-entry normals table, which is program text of the reference with an idiosyncratic triangulation: it is
neither copied nor re-derived here.  The area table (256 doubles for one spacing) is therefore an input, resolved in this order:

  1. the `area_table=` argument of the metric functions;
  2. a function registered with set_surface_area_table_fn(fn), called as fn(spacing_mm) -> 256 doubles;
  3. `metric.lookup_tables.create_table_neighbour_code_to_surface_area` of the user's own R-Super checkout, when it is importable
     (the checkout's rsuper_train directory on sys.path);
  4. otherwise an RSuperHipError that names these three ways.
"""
import importlib

import numpy as np

from ..hip.lib import RSuperHipError

ENCODE_NEIGHBOURHOOD_3D_KERNEL = np.array([[[128, 64], [32, 16]], [[8, 4], [2, 1]]])

_TABLE_FN = None


def set_surface_area_table_fn(fn):
    """Register fn(spacing_mm) -> 256 surfel areas (None removes it).  Returns the function registered before."""
    global _TABLE_FN
    old, _TABLE_FN = _TABLE_FN, fn
    return old


def _checked(table, what):
    t = np.asarray(table, dtype=np.float64)
    if t.shape != (256,):
        raise RSuperHipError(f'surface area table from {what}: expected 256 values, got shape {t.shape}')
    return np.ascontiguousarray(t)


def _checkout_table_fn():
    """create_table_neighbour_code_to_surface_area of an importable R-Super checkout, or None.  This package itself is `rsuper_amd.metric`:
    a top-level `metric` package, if there is one, is the user's."""
    try:
        mod = importlib.import_module('metric.lookup_tables')
    except Exception:
        return None
    return getattr(mod, 'create_table_neighbour_code_to_surface_area', None)


def resolve_surface_area_table(spacing_mm, area_table=None):
    """The 256 surfel areas for `spacing_mm` as a float64 numpy array, by the order in the module docstring."""
    if area_table is not None:
        if hasattr(area_table, 'detach'):
            area_table = area_table.detach().cpu().numpy()
        return _checked(area_table, 'area_table=')
    spacing = [float(s) for s in spacing_mm]
    if _TABLE_FN is not None:
        return _checked(_TABLE_FN(spacing), 'the function registered with set_surface_area_table_fn')
    fn = _checkout_table_fn()
    if fn is not None:
        return _checked(fn(spacing), 'metric.lookup_tables of the R-Super checkout')
    raise RSuperHipError(
        'no surfel area table: pass area_table= (256 doubles), register a function with '
        'rsuper_amd.metric.set_surface_area_table_fn(fn), or make your R-Super checkout importable so that '
        'metric.lookup_tables.create_table_neighbour_code_to_surface_area is found (INTEGRATION.md section 3).  The table is not part of '
        'this package and there is no CPU fallback.')
