"""Containment selection (reference: statdepth/depth/calculations/_containment.py:19-43,178-203).

The built-in definitions ('r2', 'simplex') are not Python functions here: they name
HIP kernels.  A user-supplied callable keeps the reference's plug-in protocol
`containment(data=<T x j DataFrame>, curve=<Series>, relax=<bool>) -> float`
(docs/index.md:124-148) and is evaluated by the generic enumerator in _functional.py,
on the host, because arbitrary Python cannot run on the GPU.

RANK_DEPTHS names the integrated rank depths of univariate curves (_rank.py): not band containments, but selected through
the same argument.  ORDER_DEPTHS names the depths that order the curves instead of averaging over time (the extremal
depth, _functional._extremal_depth), selected the same way.  SHAPE_DEPTHS names the depths built on the joint ranks at two
consecutive timepoints (the total variation depth and the modified shape similarity, _shape.py), selected the same way.
CLOUD_DEPTHS names the depths of the point X(t) inside the cloud of all curves' points at t, aggregated over time (the
multivariate functional halfspace depth and its projection-depth sibling, _functional._cloud_depths): the only names of
these tuples that take multivariate curves.  METRIC_DEPTHS names the depths built on the L2 distances between whole curves
(the h-modal depth, _functional._metric_depths), for univariate curves.  SPATIAL_DEPTHS names the functional spatial depth
(_functional._spatial_depths), built on the same distances and the unit vectors between whole curves, for univariate curves.
LENS_DEPTHS names the lune depths (the lens, the spherical and the beta-skeleton depth, _functional._lens_depths): counts of
the pairs of curves whose lune holds the target, read off the same distances; for univariate curves, and for point clouds
(_pointcloud._lens_cloud_depths) of any dimension.  PROJECTED_DEPTHS names the random projection depths
(_functional._projected_depths): a univariate depth of the curves' projections on a set of directions in R^T -- the random
projection depth, its Fraiman-Muniz form, the random Tukey depth and the Stahel-Donoho outlyingness over them; for
univariate curves, and through them for point clouds with any number of features.
"""
from inspect import signature

BUILTIN = ('r2', 'r2_enum', 'simplex')
RANK_DEPTHS = ('fm', 'mei', 'mhi', 'half_region', 'integrated_halfspace', 'infimal_halfspace')
ORDER_DEPTHS = ('extremal',)
SHAPE_DEPTHS = ('tvd', 'mss')
CLOUD_DEPTHS = ('halfspace', 'projection')
METRIC_DEPTHS = ('hmodal',)
SPATIAL_DEPTHS = ('spatial',)
LENS_DEPTHS = ('lens', 'spherical', 'beta_skeleton')
PROJECTED_DEPTHS = ('rp_halfspace', 'rp_fm', 'random_tukey', 'rp_projection')


def _is_valid_containment(containment):
    # a string that reaches this point is not a known definition (:34-35)
    if isinstance(containment, str):
        raise ValueError(f'containment argument \'{containment}\' is invalid. Use one of '
                         f'[\'r2\', \'r2_enum\', \'simplex \'], for univariate data one of {list(RANK_DEPTHS + ORDER_DEPTHS + SHAPE_DEPTHS + METRIC_DEPTHS + SPATIAL_DEPTHS + LENS_DEPTHS + PROJECTED_DEPTHS)}, '
                         f'for univariate or multivariate data one of {list(CLOUD_DEPTHS)}, '
                         f'or a pass a custom containment function.')
    params = signature(containment).parameters
    if len(params) != 3:   # only the arity is enforced (:37-41)
        raise ValueError('Custom containment method has incorrect number of parameters. '
                         'Expected 3, recieved {}'.format(len(params)))
    return containment


def _is_rank_depth(containment) -> bool:
    return isinstance(containment, str) and containment in RANK_DEPTHS


def _is_order_depth(containment) -> bool:
    return isinstance(containment, str) and containment in ORDER_DEPTHS


def _is_shape_depth(containment) -> bool:
    return isinstance(containment, str) and containment in SHAPE_DEPTHS


def _is_cloud_depth(containment) -> bool:
    return isinstance(containment, str) and containment in CLOUD_DEPTHS


def _is_metric_depth(containment) -> bool:
    return isinstance(containment, str) and containment in METRIC_DEPTHS


def _is_spatial_depth(containment) -> bool:
    return isinstance(containment, str) and containment in SPATIAL_DEPTHS


def _is_lens_depth(containment) -> bool:
    return isinstance(containment, str) and containment in LENS_DEPTHS


def _is_projected_depth(containment) -> bool:
    return isinstance(containment, str) and containment in PROJECTED_DEPTHS


def _select_containment(containment):
    """Returns the built-in's name, or the validated callable (:194-203)."""
    if isinstance(containment, str) and containment in BUILTIN:
        return containment
    return _is_valid_containment(containment=containment)
