from .expr import (AggExpr, And, BinComp, Col, Expr, In, IsNotNull, Lit, Not, Or,
                   col, lit, parse_predicate)
from .nodes import (Aggregate, BucketUnionNode, Filter, IndexScan, Join, LogicalPlan,
                    Project, Scan)
