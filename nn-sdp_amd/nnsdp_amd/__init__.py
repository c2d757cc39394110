"""nnsdp_amd: MI355X-native Chordal-DeepSDP LMI assembler + ADMM solver (host-side mirror of the
reference's Methods/Qc API over the C ABI in include/nnsdp.h)."""
from .methods import (  # noqa: F401
    FeedFwdNet, QcInputBox, QcSafety, QcReachHplane, QcReachCircle, QcReachEllipsoid,
    QcActivBounded, QcActivSector, SafetyQuery, ReachQuery, AdmmSdpOptions, QuerySolution,
    SingleDecomp, DoubleDecomp, DoubleRelaxDecomp, PathDecomp, AutoDecomp, DenseCone, Solver, SolverBatch, SolverFamily, same_family,
    runQuery, runQueries, solveQuery, makeZ, adjoint, makeCliques, project_psd_batched, project_psd_warm, comm_unique_id, shardPlan, certPlan, sparse_nsd,
    TARGET_OFF, TARGET_OBJECTIVE, TARGET_FEASIBLE,
)
from .frontend import (  # noqa: F401
    read_nnet, evalFeedFwdNet, evalFeedFwdNetBatch, sampleTrajs, randomNetwork, makeIntervalsInfo, makeQcActivs, approxEllipsoid,
    findEllipsoid, findCircle, findReach2Dpoly, write_scale_csv, runScale, ellipsoidQuery, makeIntervalsBatch, LiteralBounds, LiteralBoundsAlpha, CrownBounder,
    NodeBounds, makeIntervalsNodes,
)
from . import _lib  # noqa: F401
from . import vnnlib  # noqa: F401
from .vnnlib import (  # noqa: F401
    read_vnnlib, hplaneS, loadVnnlibCnf, loadReluQueriesCnf, verifyAcasSpec, verifyPairs, isSolutionGood, shardPairs, reachForm, safetyFromReach,
)
from . import split  # noqa: F401
from .split import SplitOptions, SplitResult, Leaf, verifySplit, verifySplitMany, reachSplit, ReachSplitResult, ReachLeaf, findReach2DpolySplit  # noqa: F401
from . import relusplit  # noqa: F401
from .relusplit import ReluSplitOptions, ReluLeaf, ReluSplitResult, verifyReluSplit  # noqa: F401

__version__ = "0.2.0"
