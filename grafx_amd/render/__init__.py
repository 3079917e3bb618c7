from .capture import CapturedRender, CapturedStream
from .graph import RenderState, render_grafx, silent_state
from .order.graph import compute_render_order, reorder_for_fast_render
from .prepare import RenderData, prepare_render
