from .depth import FunctionalDepth, PointcloudDepth, ProbabilisticDepth, FunctionalBoxplot, TotalVariationOutliers   # noqa: F401  (reference: statdepth/depth/__init__.py:1)
from .depth import DirectionalOutlyingness, MSPlotOutliers, CurveDistances, CurveProjections   # noqa: F401
from .calculations._helper import DepthDegeneracy     # noqa: F401
